import numpy as np
import torch

from ... import ops
from ..network import Network
from .dqn import DQN
from .native_net import NativeNet

IQN_ELIGIBLE = ("IQN runs on libjorldy_hip only: network 'iqn' with head 'mlp' and a scalar state_size, optim_config {'name': 'adam', lr, betas, eps}, "
                "1 <= num_sample <= 256, embedding_dim >= 1, 0 <= sample_min <= sample_max <= 1 (config.iqn x cartpole / mountaincar / pong_mlagent and their "
                "shapes); the cnn head (config.iqn x atari / procgen / super_mario_bros) is not on the native engine yet")


class IQNNativeNet(NativeNet):
    """`agent.network` / `agent.target_network` as the reference's IQN module is called (network/iqn.py:26-38):
    network(x, tau_min, tau_max) -> (logits [rows, N, A], tau [rows, N, 1]).  tau: use these draws ([rows, N]) instead of new ones."""

    @torch.no_grad()
    def __call__(self, x, tau_min=0, tau_max=1, tau=None):
        assert 0 <= tau_min <= tau_max <= 1
        net = self._net
        x = x.contiguous()
        outs, taus = [], []
        for o in range(0, x.shape[0], net.maxB):
            xs = x[o : o + net.maxB]
            t = net.draw_tau(int(xs.shape[0]), float(tau_min), float(tau_max)) if tau is None else tau[o : o + net.maxB].to(net.device, torch.float32).contiguous()
            outs.append(net.forward(xs, self._which, t))
            taus.append(t)
        return (outs[0] if len(outs) == 1 else torch.cat(outs, 0)), (taus[0] if len(taus) == 1 else torch.cat(taus, 0)).unsqueeze(-1)


class IQN(DQN):
    """core/agent/iqn.py:12-146: implicit quantile network.  The network (ops.IQNNet, jh_iqnnet_*) takes N sampled quantile fractions
    per row through a cosine embedding and a Hadamard product with the state embedding; the online net selects the next action by the
    mean over the samples, the target net evaluates it; pairwise quantile-Huber loss weighted by the FIRST forward's fractions
    (jh_iqn_loss).  Acting is jh_iqn_act.  As in the reference (iqn.py:44-49) the network is 512 wide whatever hidden_size says."""

    WIDTH = 512  # network/iqn.py:10: D_hidden's default, which the agent never overrides

    def __init__(self, state_size, action_size, network="iqn", head="mlp", optim_config={"name": "adam"}, num_sample=64, embedding_dim=64, sample_min=0.0,
                 sample_max=1.0, **kwargs):
        got = (f"; got network={network!r}, head={head!r}, state_size={state_size!r}, optim_config={optim_config!r}, num_sample={num_sample!r}, "
               f"embedding_dim={embedding_dim!r}, sample_min={sample_min!r}, sample_max={sample_max!r}")
        ok_opt = optim_config.get("name", "adam").lower() == "adam" and set(optim_config) <= {"name", "lr", "betas", "eps"}
        ok_n = isinstance(num_sample, (int, np.integer)) and 1 <= num_sample <= 256 and isinstance(embedding_dim, (int, np.integer)) and embedding_dim >= 1
        if not (network == "iqn" and head == "mlp" and np.isscalar(state_size) and ok_opt and ok_n and 0 <= sample_min <= sample_max <= 1):
            raise ValueError(IQN_ELIGIBLE + got)
        self.num_support = int(num_sample)
        self.embedding_dim = int(embedding_dim)
        self.sample_min = float(sample_min)
        self.sample_max = float(sample_max)
        self._tau_inject = None  # test hook: the tau draws of the next learn() ([3, B, N]) / act() ([rows, N]) instead of torch.rand
        super().__init__(state_size, action_size, network=network, head=head, optim_config=optim_config, **kwargs)
        self._stats8 = self._mapped_stats(8)

    # ---- the construction hooks of DQN / NativeValueNetMixin: the network is IQN's own, no q-network is built and thrown away (iqn.py:41-49 does)
    def _require_native(self, backend, network, head, state_size, hidden_size, optim_config):
        if backend not in (None, "auto", "native"):
            raise ValueError(f"backend={backend!r}: jorldy_amd has one backend (libjorldy_hip); {IQN_ELIGIBLE}")

    def _initial_net(self, network, state_size, action_size, hidden_size, head):
        return Network(network, state_size, action_size, self.embedding_dim, self.num_support, head=head)  # iqn.py:44-46: hidden_size is not passed

    _net_view = IQNNativeNet

    def _build_native_net(self, network, state_size, action_size, num_support, hidden_size, head, batch_size, noise_type):
        return ops.IQNNet(state_size, action_size, self.embedding_dim, self.num_support, self.WIDTH, batch_size, self.device)

    def logits2Q(self, logits):
        _logits = torch.transpose(logits, 1, 2).contiguous()
        return _logits, torch.mean(_logits, dim=-1)

    @torch.no_grad()
    def act(self, state, training=True):
        self.network.train(training)
        epsilon = self.epsilon if training else self.epsilon_eval
        sample_min = 0.0 if training else self.sample_min
        sample_max = 1.0 if training else self.sample_max
        if np.random.random() < epsilon:
            batch_size = state[0].shape[0] if isinstance(state, list) else state.shape[0]
            action = np.random.randint(0, self.action_size, size=(batch_size, 1))
        else:
            self._net.tau_range, self._net.tau_inject = (sample_min, sample_max), self._tau_inject
            try:
                action = self._act_greedy(state)
                if action is None:
                    logits, _ = self.network(self.as_tensor(state), sample_min, sample_max)
                    _, q_action = self.logits2Q(logits)
                    action = torch.argmax(q_action, -1, keepdim=True).cpu().numpy()
            finally:
                self._net.tau_range, self._net.tau_inject = (0.0, 1.0), None
        return {"action": action}

    def _act_kernel(self, logits, out):
        # _act_greedy hands the output buffer over viewed [rows, A, K]; the network wrote it as [rows, N, A]
        ops.iqn_act(logits.view(logits.shape[0], self.num_support, self.action_size), out=out)

    def _alloc_static(self):
        st = self._alloc_static_native()
        B, N, A = self.batch_size, self.num_support, self.action_size
        st["logits"] = torch.empty(3, B, N, A, dtype=torch.float32, device=self.device)
        st["tau"] = torch.zeros(3, B, N, dtype=torch.float32, device=self.device)
        return st

    def _draw(self, st):
        """The sampled rows, then the three tau sets of this learn() (iqn.py:90, 100, 103: one uniform draw per forward), eagerly into the
        static buffer the captured body reads: a replayed graph sees fresh draws."""
        super()._draw(st)
        if self._tau_inject is not None:
            st["tau"].copy_(torch.as_tensor(self._tau_inject).to(self.device, torch.float32).reshape(st["tau"].shape))
        else:
            torch.rand(st["tau"].shape, out=st["tau"])

    def _learn_body(self, st):
        B = self.batch_size
        net = self._net
        tr = self.memory.gather(st["idx"], as_float=self._as_float(), out=st["tr"])
        lg = net.learn_forward(st["x_all"], B, st["tau"], st["logits"])
        g, _ = ops.iqn_loss(lg[0], lg[1], lg[2], tr["action"], tr["reward"], tr["done"], st["tau"][0], self.gamma, stats=self._stats8.dev)
        net.backward(g)
        if self.grad_sync is not None:
            self.grad_sync.reduce_flat(net.grads)
        net.optim_step(self._opt_name, self.clip_grad_norm)

    def learn(self):
        s, _ = self._learn_stats(self._stats8, (5, 7))
        return {"loss": float(s[0]), "epsilon": self.epsilon, "max_Q": float(s[1]), "max_logit": float(s[2]), "min_logit": float(s[3])}
