from ... import ops
from .dqn import DQN

M_ELIGIBLE = ("MDQN runs on libjorldy_hip only: network 'discrete_q_network' or 'dueling' with head 'mlp' (scalar state_size) or head 'cnn' ((C, H, W) state_size), "
              "hidden_size % 4 == 0, optim_config {'name': 'adam', lr, betas, eps} or {'name': 'rmsprop', lr, alpha, eps, centered}, tau > 0, l_0 <= 0 "
              "(config.m_dqn x cartpole / mountaincar / pong_mlagent / atari / procgen and their shapes); "
              "a noisy 'rainbow' network has no Munchausen form in the reference")


class MDQN(DQN):
    """core/agent/m_dqn.py:10-72: Munchausen DQN.  The target adds alpha * clip(tau log pi(a|s), l_0, 0) of the TARGET network's
    softmax policy at the taken action to the reward and bootstraps from the soft value of target(s').  The three forwards
    online(s), target(s), target(s') are one pass (jh_rbnet_learn_forward_m: the target trunk runs over both halves of the batch),
    the loss with its gradient is one HIP kernel (jh_mdqn_loss); everything else is DQN's native path."""

    def __init__(self, alpha=0.9, tau=0.03, l_0=-1, **kwargs):
        network = kwargs.get("network", "discrete_q_network")
        if network not in ("discrete_q_network", "dueling"):
            raise ValueError(f"{M_ELIGIBLE}; got network={network!r}")
        if not tau > 0:
            raise ValueError(f"{M_ELIGIBLE}; got tau={tau!r}")
        if not l_0 <= 0:
            raise ValueError(f"{M_ELIGIBLE}; got l_0={l_0!r}")
        super().__init__(**kwargs)
        self.alpha = alpha
        self.tau = tau
        self.l_0 = l_0
        self._net.reserve_target_rows(2 * self.batch_size)  # target(s) and target(s') share the target slot; allocated here, not inside a captured learn()

    def _learn_body(self, st):
        net, B, A = self._net, self.batch_size, self.action_size
        tr = self.memory.gather(st["idx"], as_float=self._as_float(), out=st["tr"])
        lg = net.learn_forward_m(st["x_all"], B, None, st["logits"])  # online(s), target(s), target(s') in shared launches
        g, _ = ops.mdqn_loss(lg[0].view(B, A), lg[1].view(B, A), lg[2].view(B, A), tr["action"], tr["reward"], tr["done"], self.gamma, self.alpha, self.tau,
                             self.l_0, stats=self._stats.dev)
        net.backward(g)
        if self.grad_sync is not None:  # data-parallel learners: one all-reduce of the flat gradient bucket
            self.grad_sync.reduce_flat(net.grads)
        net.optim_step(self._opt_name, self.clip_grad_norm)

    def learn(self):
        s, _ = self._learn_stats(self._stats, (3,))
        return {"loss": float(s[0]), "epsilon": self.epsilon, "max_Q": float(s[1])}
