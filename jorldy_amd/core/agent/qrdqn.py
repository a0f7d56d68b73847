import numpy as np
import torch

from ... import ops
from .dqn import DQN

QR_ELIGIBLE = ("QRDQN runs on libjorldy_hip only: network 'discrete_q_network' with head 'mlp' (scalar state_size) or head 'cnn' ((C, H, W) state_size), "
               "hidden_size % 4 == 0, optim_config {'name': 'adam', lr, betas, eps} or {'name': 'rmsprop', lr, alpha, eps, centered}, "
               "1 <= num_support <= 256 (config.qrdqn x cartpole / mountaincar / pong_mlagent / atari / procgen and their shapes); "
               "the dueling combine over action_size * num_support pseudo-actions has no meaning for quantiles")


def quantile_midpoints(num_support):
    """tau of qrdqn.py:26-31 as float32 [num_support]: the SAME torch.arange call on the CPU (in float32 it is one ulp away from
    (2 i + 1) / (2 N) in places, so it is not recomputed anywhere else).  For some num_support that arange has num_support + 1
    elements and the reference's .view(1, num_support) raises: ValueError here."""
    n = int(num_support)
    if n < 1:
        raise ValueError(f"num_support={num_support!r}: QRDQN needs at least one quantile")
    min_tau = 1 / (2 * n)
    max_tau = (2 * n + 1) / (2 * n)
    tau = torch.arange(min_tau, max_tau, 1 / n)
    if tau.numel() != n:
        raise ValueError(f"num_support={n}: torch.arange({min_tau}, {max_tau}, {1 / n}) has {tau.numel()} elements, not {n} (floating-point end point); "
                         "the reference's tau.view(1, num_support) raises for this value too -- pick a neighbouring num_support")
    return tau.to(torch.float32).contiguous()


class QRDQN(DQN):
    """core/agent/qrdqn.py:10-115: quantile-regression DQN.  The q-network's A * N outputs are N quantiles per action; the online
    net selects the next action by the quantile means, the target net evaluates it; pairwise quantile-Huber loss.  The loss with
    its gradient is one HIP kernel (jh_qr_loss), acting is jh_quantile_act; everything else is DQN's native path."""

    def __init__(self, state_size, action_size, num_support=200, **kwargs):
        network = kwargs.get("network", "discrete_q_network")
        if network != "discrete_q_network":
            raise ValueError(f"{QR_ELIGIBLE}; got network={network!r}")
        tau = quantile_midpoints(num_support)
        if num_support > 256:
            raise ValueError(f"{QR_ELIGIBLE}; got num_support={num_support}")
        super().__init__(state_size, action_size * num_support, **kwargs)
        self.action_size = action_size
        self.num_support = num_support
        self.tau = tau.to(self.device).view(1, num_support)
        self.inv_tau = 1 - self.tau
        self._stats8 = self._mapped_stats(8)

    def logits2Q(self, logits):
        _logits = logits.view(logits.shape[0], self.action_size, self.num_support)
        return _logits, torch.mean(_logits, dim=-1)

    @torch.no_grad()
    def act(self, state, training=True):
        self.network.train(training)
        epsilon = self.epsilon if training else self.epsilon_eval
        if np.random.random() < epsilon:
            batch_size = state[0].shape[0] if isinstance(state, list) else state.shape[0]
            action = np.random.randint(0, self.action_size, size=(batch_size, 1))
        else:
            action = self._act_greedy(state)
            if action is None:
                _, q_action = self.logits2Q(self.network(self.as_tensor(state)))
                action = torch.argmax(q_action, -1, keepdim=True).cpu().numpy()
        return {"action": action}

    def _act_kernel(self, logits, out):
        ops.quantile_act(logits, out=out)

    def _learn_body(self, st):
        B, A, N = self.batch_size, self.action_size, self.num_support
        net = self._net  # q-network with A*N outputs on the native engine
        tr = self.memory.gather(st["idx"], as_float=self._as_float(), out=st["tr"])
        lg = net.learn_forward(st["x_all"], B, None, st["logits"])
        g, _ = ops.qr_loss(lg[0].view(B, A, N), lg[1].view(B, A, N), lg[2].view(B, A, N), tr["action"], tr["reward"], tr["done"], self.tau, self.gamma,
                           stats=self._stats8.dev)
        net.backward(g.view(B, A * N))
        if self.grad_sync is not None:
            self.grad_sync.reduce_flat(net.grads)
        net.optim_step(self._opt_name, self.clip_grad_norm)

    def learn(self):
        s, _ = self._learn_stats(self._stats8, (5, 7))
        return {"loss": float(s[0]), "epsilon": self.epsilon, "max_Q": float(s[1]), "max_logit": float(s[2]), "min_logit": float(s[3])}
