from ... import ops
from .iqn import IQN, IQN_ELIGIBLE

MIQN_ELIGIBLE = "M-IQN's Munchausen target needs tau > 0 and l_0 <= 0 (config.m_iqn.*: alpha 0.9, tau 0.03, l_0 -1); " + IQN_ELIGIBLE


class MIQN(IQN):
    """core/agent/m_iqn.py:10-110: Munchausen IQN.  IQN's network and pairwise quantile-Huber loss under M-DQN's target: alpha *
    clip(tau log pi(a|s), l_0, 0) is added to the reward and every target quantile bootstraps from the soft value of target(s').  Unlike
    M-DQN, the policy of the bonus is the ONLINE network's, from a forward of its own with a fresh draw (m_iqn.py:50-51).  The
    reference's four forwards are three here (jh_iqnnet_learn_forward_m: its online(next_state) feeds nothing), the loss with its
    gradient is jh_miqn_loss; acting, checkpoints, weight sync and lr decay are IQN's."""

    def __init__(self, alpha=0.9, tau=0.03, l_0=-1, **kwargs):
        if not tau > 0:
            raise ValueError(f"{MIQN_ELIGIBLE}; got tau={tau!r}")
        if not l_0 <= 0:
            raise ValueError(f"{MIQN_ELIGIBLE}; got l_0={l_0!r}")
        super().__init__(**kwargs)
        self.alpha = alpha
        self.tau = tau
        self.l_0 = l_0

    def _learn_body(self, st):
        """st["tau"] [3, B, N] in the native slot order: online(state) for the loss, online(state) for the policy, target(next_state) --
        the reference's draws 0, 3 and 2 (its draw 1 goes to the forward that is not run)."""
        B = self.batch_size
        net = self._net
        tr = self.memory.gather(st["idx"], as_float=self._as_float(), out=st["tr"])
        lg = net.learn_forward_m(st["x_all"], B, st["tau"], st["logits"])
        g, _ = ops.miqn_loss(lg[0], lg[1], lg[2], tr["action"], tr["reward"], tr["done"], st["tau"][0], self.gamma, self.alpha, self.tau, self.l_0, stats=self._stats8.dev)
        net.backward(g)
        if self.grad_sync is not None:
            self.grad_sync.reduce_flat(net.grads)
        net.optim_step(self._opt_name, self.clip_grad_norm)
