import numpy as np
import torch

from ... import ops
from ..network import Network
from .dqn import DQN
from .native_net import NoiseDrawMixin, native_supported

# The networks the Noisy agent may run, and the engine kind behind each.  A table of its own: "noisy" stays refused for every other agent
# (dqn, per, ape_x, m_dqn, ...), whose learn() the reference cannot run on this network either (no `is_train` argument there).
_NOISY_KIND_OF = {"noisy": "noisy"}

NOISY_ELIGIBLE = ("the Noisy agent runs on libjorldy_hip only: network 'noisy' (factorized | independent noise), "
                  "head 'mlp' with a scalar state_size or head 'cnn' with a (C, H, W) state_size, hidden_size % 4 == 0, optim_config "
                  "{'name': 'adam', lr, betas, eps} or {'name': 'rmsprop', lr, alpha, eps, centered} "
                  "(config.noisy x cartpole / mountaincar / pong_mlagent / atari / procgen / super_mario_bros and their shapes)")


class Noisy(NoiseDrawMixin, DQN):
    """core/agent/noisy.py:12-144: DQN that explores through NoisyNet layers instead of epsilon-greedy.  learn(): uniform sample -> fused
    gather -> one noise draw per forward -> online(s; noise 0), target(s'; noise 1) in shared launches (jh_rbnet_learn_forward_n: two
    forwards, not DQN's three) -> jh_td_loss (max target, Huber mean) -> backward with d(sig) = d(mu) * eps -> optimizer -> mean |sig_w|
    of both layers (jh_rbnet_sig_abs_mean), all replayed as one hipGraph; one read-back.

    The network is engine kind 4 / 5 (ops.RainbowNet(kind="noisy")): head -> noisy(F -> H) -> relu -> noisy(H -> A), mlp / cnn head, plain
    Adam / RMSprop.  One backend: any other configuration raises (NOISY_ELIGIBLE)."""

    def __init__(self, state_size, action_size, hidden_size=512, network="noisy", head="mlp", optim_config={"name": "adam"}, noise_type="factorized",
                 **kwargs):
        self.noise_type = noise_type
        super().__init__(state_size, action_size, hidden_size=hidden_size, network=network, head=head, optim_config=optim_config, **kwargs)
        self._stats8 = self._mapped_stats(8)  # [0:4] jh_td_loss's, [4:6] the sigma means (written last)

    def _require_native(self, backend, network, head, state_size, hidden_size, optim_config):
        if backend not in (None, "auto", "native"):
            raise ValueError(f"backend={backend!r}: jorldy_amd has one backend (libjorldy_hip)")
        ok = (network in _NOISY_KIND_OF and self.noise_type in ("factorized", "independent")
              and native_supported("discrete_q_network", head, state_size, hidden_size, optim_config))  # head / state / hidden / optimizer: DQN's rules
        if not ok:
            raise ValueError(f"{NOISY_ELIGIBLE}; got network={network!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size}, "
                             f"noise_type={self.noise_type!r}, optim_config={optim_config!r}")

    def _initial_net(self, network, state_size, action_size, hidden_size, head):
        """The reference constructs the network four times -- DQN.__init__'s pair (dqn.py:72-78, default noise type), then Noisy.__init__'s pair
        (noisy.py:47-63) -- and keeps the third: the same constructions in the same order, so one torch.manual_seed gives its weights."""
        for _ in range(2):
            Network(network, state_size, action_size, D_hidden=hidden_size, head=head)
        kept = Network(network, state_size, action_size, self.noise_type, D_hidden=hidden_size, head=head)
        Network(network, state_size, action_size, self.noise_type, D_hidden=hidden_size, head=head)  # target_network: overwritten by load_state_dict
        return kept

    def _build_native_net(self, network, state_size, action_size, num_support, hidden_size, head, batch_size, noise_type):
        return ops.RainbowNet(state_size, action_size, num_support, hidden_size, head, batch_size, self.device, kind=_NOISY_KIND_OF[network],
                              noise_type=self.noise_type)

    @torch.no_grad()
    def act(self, state, training=True):
        """noisy.py:67-81: uniform random actions until learning starts (one np.random.randint, no epsilon draw), then greedy on the noisy
        network -- a fresh noise draw per call when training, mu only in evaluation."""
        self.network.train(training)
        if training and self.memory.size < max(self.batch_size, self.start_train_step):
            rows = state[0].shape[0] if isinstance(state, list) else state.shape[0]
            action = np.random.randint(0, self.action_size, size=(rows, 1))
        else:
            action = self._act_greedy(state, training)
            if action is None:
                action = torch.argmax(self.network(self.as_tensor(state), training), -1, keepdim=True).cpu().numpy()
        return {"action": action}

    def _alloc_static(self):
        st = self._alloc_static_native()
        st["noise"] = torch.zeros(2, self._net.noise_len, dtype=torch.float32, device=self.device)  # network(s), target_network(s')
        return st

    def _learn_body(self, st):
        net, B, A = self._net, self.batch_size, self.action_size
        tr = self.memory.gather(st["idx"], idx_offset=0, as_float=self._as_float(), out=st["tr"])
        self._draw_noise(st)
        lg = net.learn_forward_n(st["x_all"], B, st["noise"], st["logits"])  # online(s; noise 0), target(s'; noise 1)
        g, _, _ = ops.td_loss(lg[0].view(B, A), lg[1].view(B, A), tr["action"], tr["reward"], tr["done"], self.gamma, stats=self._stats8.dev[:4])
        net.backward(g, defer=self.grad_sync is None)  # d(sig) = d(mu) * eps and conv1's partial sums wait for the optimizer step
        if self.grad_sync is not None:  # data-parallel learners: one all-reduce of the flat gradient bucket
            self.grad_sync.reduce_flat(net.grads)
        net.optim_step(self._opt_name, self.clip_grad_norm)
        net.sig_abs_mean(self._stats8.dev[4:6])  # after the step, like the reference (noisy.py:113)

    def learn(self):
        s, _ = self._learn_stats(self._stats8, (5,))
        return {"loss": float(s[0]), "max_Q": float(s[1]), "sig_w1": float(s[4]), "sig_w2": float(s[5])}

    def process(self, transitions, step):
        """noisy.py:124-144: DQN's without the epsilon decay."""
        result = {}
        self._store(transitions)
        delta_t = step - self.time_t
        self.time_t = step
        self.target_update_stamp += delta_t
        if self.memory.size >= self.batch_size and self.time_t >= self.start_train_step:
            result = self.learn()
            if self.lr_decay:
                self.learning_rate_decay(step)
        if self.num_learn > 0 and self.target_update_stamp >= self.target_update_period:
            self.update_target()
            self.target_update_stamp -= self.target_update_period
        return result

