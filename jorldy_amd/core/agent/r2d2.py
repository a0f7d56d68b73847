from collections import deque
from itertools import islice

import numpy as np
import torch

from ... import ops
from ..network import Network
from .dqn import ApeX
from .native_net import NativeNet

MAX_BATCH, MAX_SEQ, MAX_ACTIONS = 1024, 128, 64  # jh_r2d2_loss: one workgroup, one batch row per thread looping over the trained steps
R2D2_ELIGIBLE = ("R2D2 runs on libjorldy_hip only: network 'r2d2' with head 'mlp' and a scalar state_size, hidden_size % 4 == 0, "
                 f"2 <= action_size <= {MAX_ACTIONS}, 0 < n_burn_in < seq_len <= {MAX_SEQ}, n_step >= 1, batch_size <= {MAX_BATCH}, optim_config "
                 "{'name': 'adam', lr, betas, eps} (config.r2d2.cartpole / pong_mlagent and their shapes); the cnn head (config.r2d2.atari), "
                 "frame_dedup and data-parallel learners (grad_sync) are not available for this agent")


class R2D2NativeNet(NativeNet):
    """`agent.network` / `agent.target_network` as the reference's R2D2 module is called (network/r2d2.py:28-53):
    network(x1 [N, T, S], x2 [N, T, A], hidden_in=(h, c) each [1, N, H] or None) -> (q [N, T, A], hidden_in, hidden_out), one native step
    launch chain per time step (ops.R2D2Net.act_step).  Online parameters only: the target network is evaluated inside learn()."""

    @torch.no_grad()
    def __call__(self, x1, x2, hidden_in=None):
        net = self._net
        if self._which != 0:
            raise ValueError("the target network of R2D2 is evaluated inside learn() only")
        x1, x2 = x1.to(net.device, torch.float32), x2.to(net.device, torch.float32)
        N, T = int(x1.shape[0]), int(x1.shape[1])
        if hidden_in is None:
            hidden_in = (torch.zeros(1, N, net.H, device=net.device), torch.zeros(1, N, net.H, device=net.device))
        h, c = hidden_in[0][0].contiguous(), hidden_in[1][0].contiguous()
        qs = []
        for t in range(T):
            q, h, c = net.act_step(x1[:, t].contiguous(), x2[:, t].contiguous(), h, c)
            qs.append(q)
        return torch.stack(qs, 1), hidden_in, (h[None], c[None])


class R2D2(ApeX):
    """core/agent/r2d2.py:12-313: Recurrent Replay Distributed DQN on the native engine.

      network       ops.R2D2Net (jh_r2d2net_*): head -> cat[x, prev_action_onehot] -> LSTM -> l -> dueling streams over flat buckets.
      replay        Ape-X's PER buffer with actor-side priorities; a stored row holds whole windows (state [L, S], prev_action_onehot [L, A],
                    action / reward / done [L - 1, 1], the LSTM state at the window's start and n_step later; L = seq_len + n_step), emitted by
                    interact_callback every seq_len // 2 steps and at once after an episode start, left-padded with zeros when zero_padding.
      learn()       gather -> the three sequence passes in lockstep (one LSTM step launch per time step serves all three) -> jh_r2d2_loss
                    (double-Q selection, both value rescales, the n-step fold, the sequence priorities in float64, the LAST trained step's
                    IS-weighted loss) -> priority write-back -> backpropagation through time over the trained steps -> clip + Adam.  One
                    hipGraph after a warm eager call, one stream, no branches.  beta is annealed once more here, as in the reference.
      act()         one step with the carried (h, c) and the previous action's one-hot, both kept on the device.

    Departures on purpose: both value rescales are evaluated without their cancellation -- sqrt(1 + y) - 1 inside the inverse (the reference's
    float32 expression loses up to 2e-4 of the largest target at small |Q|) and sqrt(|x| + 1) - 1 inside the forward one --, in double; act() with more than one row returns each row's OWN q where the
    reference's np.take(q, action) reads the flattened array (identical at one row)."""

    def __init__(self, state_size, action_size, network="r2d2", head="mlp", hidden_size=512, optim_config={"name": "adam"}, batch_size=64, n_step=4,
                 seq_len=80, n_burn_in=40, zero_padding=True, eta=0.9, frame_dedup=False, **kwargs):
        is_int = lambda v: isinstance(v, (int, np.integer))
        ok = (network == "r2d2" and head == "mlp" and np.isscalar(state_size) and is_int(hidden_size) and hidden_size >= 4 and hidden_size % 4 == 0
              and is_int(action_size) and 2 <= action_size <= MAX_ACTIONS and is_int(seq_len) and is_int(n_burn_in) and 0 < n_burn_in < seq_len <= MAX_SEQ
              and is_int(n_step) and 1 <= n_step <= MAX_SEQ and is_int(batch_size) and 1 <= batch_size <= MAX_BATCH and isinstance(optim_config, dict)
              and str(optim_config.get("name", "adam")).lower() == "adam" and set(optim_config) <= {"name", "lr", "betas", "eps"}
              and not frame_dedup and kwargs.get("grad_sync") is None)
        if not ok:
            raise ValueError(f"{R2D2_ELIGIBLE}; got network={network!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size!r}, "
                             f"action_size={action_size!r}, seq_len={seq_len!r}, n_burn_in={n_burn_in!r}, n_step={n_step!r}, batch_size={batch_size!r}, "
                             f"optim_config={optim_config!r}, frame_dedup={frame_dedup!r}, grad_sync={kwargs.get('grad_sync')!r}")
        kwargs.pop("grad_sync", None)
        self.seq_len, self.n_burn_in, self.zero_padding, self.eta = int(seq_len), int(n_burn_in), zero_padding, eta
        self._n_step_net = int(n_step)
        super().__init__(state_size=state_size, action_size=action_size, network=network, head=head, hidden_size=hidden_size, optim_config=optim_config,
                         batch_size=batch_size, n_step=n_step, **kwargs)
        self.hidden_size = int(hidden_size)
        self.hidden = None        # (h, c) each [1, N, H] on the device
        self.prev_action = None
        self.tmp_buffer = deque(maxlen=self.n_step + self.seq_len)
        self.store_period = self.seq_len // 2
        self.store_period_stamp = 0
        self.store_start = True
        self.memory.defer_rows = 0  # rows are whole windows: straight into the ring
        self._stats8 = self._mapped_stats(8)

    # ---- the construction hooks of DQN / NativeValueNetMixin
    def _require_native(self, backend, network, head, state_size, hidden_size, optim_config):
        if backend not in (None, "auto", "native"):
            raise ValueError(f"backend={backend!r}: jorldy_amd has one backend (libjorldy_hip); {R2D2_ELIGIBLE}")

    def _initial_net(self, network, state_size, action_size, hidden_size, head):
        return Network(network, state_size, action_size, D_hidden=hidden_size, head=head)

    _net_view = R2D2NativeNet

    def _build_native_net(self, network, state_size, action_size, num_support, hidden_size, head, batch_size, noise_type):
        return ops.R2D2Net(state_size, action_size, hidden_size, batch_size, self.seq_len, self.n_burn_in, self._n_step_net, self.device)

    # ---------------------------------------------------------------------------------- acting
    @torch.no_grad()
    def act(self, state, training=True):
        """r2d2.py:47-90.  The draws are the reference's, in its order: np.random.random(), then randint.  `q` is each row's own Q of the
        action taken; the carried state and the previous action's one-hot stay on the device between calls."""
        self.network.train(training)
        epsilon = self.epsilon if training else self.epsilon_eval
        net, A = self._net, self.action_size
        x = self.as_tensor(np.asarray(state, dtype=np.float32)).contiguous()
        N = int(x.shape[0])
        if self.prev_action is None:
            onehot_out = np.zeros((N, A), np.float32)  # r2d2.py:52-60: float32 zeros at an episode start, F.one_hot's int64 afterwards
        else:
            onehot_out = np.eye(A, dtype=np.int64)[np.asarray(self.prev_action).reshape(N)]
        onehot = self.as_tensor(onehot_out.astype(np.float32))
        if self.hidden is None:
            self.hidden = (torch.zeros(1, N, net.H, device=self.device), torch.zeros(1, N, net.H, device=self.device))
        hidden_in = self.hidden
        q, h, c = net.act_step(x, onehot, hidden_in[0][0], hidden_in[1][0])
        greedy, _, _ = ops.value_act(q.view(N, A, 1))  # first maximum, like torch.argmax
        q_host = q.cpu().numpy()
        if np.random.random() < epsilon:
            action = np.random.randint(0, A, size=(N, 1))
        else:
            action = greedy.cpu().numpy().reshape(N, 1)
        self.hidden = (h[None], c[None])
        self.prev_action = action
        return {"action": action, "prev_action_onehot": onehot_out, "q": np.take_along_axis(q_host, action, axis=1),
                "hidden_h": hidden_in[0].cpu().numpy(), "hidden_c": hidden_in[1].cpu().numpy()}

    def interact_callback(self, transition):
        """r2d2.py:179-287, host numpy as written."""
        _transition = {}
        self.tmp_buffer.append(transition)

        if (self.store_start or self.store_period_stamp == self.store_period) and (
            (self.zero_padding and len(self.tmp_buffer) >= self.n_step + 1) or (not self.zero_padding and len(self.tmp_buffer) == self.tmp_buffer.maxlen)
        ):
            _transition["hidden_h"] = self.tmp_buffer[0]["hidden_h"]
            _transition["hidden_c"] = self.tmp_buffer[0]["hidden_c"]
            _transition["next_hidden_h"] = self.tmp_buffer[self.n_step]["hidden_h"]
            _transition["next_hidden_c"] = self.tmp_buffer[self.n_step]["hidden_c"]

            for key in self.tmp_buffer[0].keys():
                if key not in ["hidden_h", "hidden_c", "next_state"]:
                    if key in ["q", "state", "prev_action_onehot"]:
                        _transition[key] = np.stack([t[key] for t in self.tmp_buffer], axis=1)
                    else:
                        _transition[key] = np.stack([t[key] for t in self.tmp_buffer][:-1], axis=1)

            # state sequence zero padding
            if self.zero_padding and len(self.tmp_buffer) < self.tmp_buffer.maxlen:
                lack_dims = self.tmp_buffer.maxlen - len(self.tmp_buffer)
                for key in ("state", "prev_action_onehot", "action", "reward", "done", "q"):
                    zero = np.zeros((1, lack_dims, *transition[key].shape[1:]))
                    _transition[key] = np.concatenate((zero, _transition[key]), axis=1)
                k = 0 if lack_dims > self.n_step else self.n_step - lack_dims
                _transition["next_hidden_h"] = self.tmp_buffer[k]["hidden_h"]
                _transition["next_hidden_c"] = self.tmp_buffer[k]["hidden_c"]

            target_q = self.inv_val_rescale(_transition["q"][:, self.n_burn_in + self.n_step:])
            for i in reversed(range(self.n_step)):
                target_q = (_transition["reward"][:, i + self.n_burn_in:i + self.seq_len]
                            + (1 - _transition["done"][:, i + self.n_burn_in:i + self.seq_len]) * self.gamma * target_q)
            target_q = self.val_rescale(target_q)
            td_error = abs(target_q - _transition["q"][:, self.n_burn_in:self.seq_len])
            priority = self.eta * np.max(td_error, axis=1) + (1 - self.eta) * np.mean(td_error, axis=1)
            _transition["priority"] = priority
            del _transition["q"]

            self.store_start = False
            self.store_period_stamp -= self.store_period

        if len(self.tmp_buffer) > self.n_step and self.tmp_buffer[-self.n_step - 1]["done"]:
            self.store_start = True
            self.tmp_buffer = deque(islice(self.tmp_buffer, len(self.tmp_buffer) - self.n_step, None), maxlen=self.tmp_buffer.maxlen)

        self.store_period_stamp += 1
        if transition["done"]:
            self.hidden = None
            self.prev_action = None

        return _transition

    def val_rescale(self, val, eps=1e-3):
        return (val / (abs(val) + 1e-10)) * ((abs(val) + 1) ** (1 / 2) - 1) + (eps * val)

    def inv_val_rescale(self, val, eps=1e-3):
        return (val / (abs(val) + 1e-10)) * ((((1 + 4 * eps * (abs(val) + 1 + eps)) ** (1 / 2) - 1) / (2 * eps)) ** 2 - 1)

    # ---------------------------------------------------------------------------------- learn
    def _alloc_static(self):
        """Fixed-address buffers of one learn(): sampled tree indices, IS weights, the gathered windows, the three passes' Q values."""
        B = self.batch_size
        idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        tr = dict(self.memory.gather(idx, idx_offset=0, as_float=True))
        L = self.seq_len + self.n_step
        assert tuple(tr["state"].shape[:2]) == (B, L) and tuple(tr["action"].shape[:2]) == (B, L - 1), "stored rows are not seq_len + n_step windows"
        return dict(idx=idx, w=torch.ones(B, dtype=torch.float32, device=self.device), tr=tr, store=self.memory._store,
                    q=torch.empty(3, self.seq_len - self.n_burn_in, B, self.action_size, dtype=torch.float32, device=self.device))

    def _learn_body(self, st):
        net = self._net
        tr = self.memory.gather(st["idx"], idx_offset=self._idx_offset(), as_float=True, out=st["tr"])
        q = net.learn_forward(tr["state"], tr["prev_action_onehot"], tr["hidden_h"], tr["hidden_c"], tr["next_hidden_h"], tr["next_hidden_c"], out=st["q"])
        g, prio, _, _ = ops.r2d2_loss(q[0], q[1], q[2], tr["action"], tr["reward"], tr["done"], st["w"], self.n_burn_in, self.n_step, self.gamma, self.eta, self.alpha,
                                      stats=self._stats8.dev)
        self.memory.update_priorities(st["idx"], prio)
        net.backward(g)
        net.optim_step(self._opt_name, self.clip_grad_norm)

    def learn(self):
        if self.grad_sync is not None:
            raise ValueError(R2D2_ELIGIBLE)
        s, p = self._learn_stats(self._stats8, (5, 7))
        self.beta = min(1.0, self.beta + self.beta_add)  # r2d2.py:153, on top of process()'s
        return {"loss": float(s[0]), "max_Q": float(s[1]), "sampled_p": float(p[0]), "mean_p": float(p[1]), "num_learn": self.num_learn,
                "num_transitions": self.num_transitions}
