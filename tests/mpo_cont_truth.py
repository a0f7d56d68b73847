"""Float64 numpy statement of the contracts of jh_mpo_sample and jh_mpo_loss_continuous (include/jorldy_hip.h; core/agent/mpo.py:199-309 and
416-419 for a continuous policy): the comparator of tests/test_mpo_continuous_cpu.py and tests/test_mpo_continuous_gpu.py (test infrastructure,
not the product).  Inputs are float32 arrays; everything after them is float64.

  sample             zn, zt_add and their tanh from the raw heads and the standard normals
  loss               log_prob and c of the stored action, Qret before and after the Retrace scan, At, the E-step weights over the samples, KLD_mu,
                     KLD_sigma, the four losses, d(loss)/d(raw head of online(s)), d(loss)/d(q), the gradients of all three multipliers and the
                     extrema of q and At
  loss_torch         the SAME quantities the way the reference writes them -- Normal.log_prob, exp(At / eta) without the row maximum, the log of
                     the ratio of the products -- with torch autograd in a given dtype: float32 is the comparator whose own error against float64
                     the acceptance rule of the GPU tests needs, float64 cross-checks `loss`
and the case builders of the kernel tests.  The multipliers' Adam step is tests/mpo_truth.py's multiplier_step."""
import os
from collections import OrderedDict

import numpy as np

from mpo_truth import GOLDEN, NAMES, STATS, multiplier_step, recipe_weights, thin  # noqa: F401  (re-exported: one statement of the step)

HALF_LOG_2PI = 0.91893853320467274178
ATANH_BOUND = float(np.float32(1.0 - 1e-7))  # the reference clamps the float32 action tensor: the bound as float32 rounds it
# the kernel tests' optimizer block
LR, BETAS, ADAM_EPS, STEP0 = 3e-3, (0.9, 0.999), 1e-8, 4
# (R, T, N, A).  The first four are the sampling kernel's: one row, a ragged wavefront, just over one wavefront with T = 1, four wavefronts at
# pendulum's N.  The loss kernel adds hopper-like N * R = 7680 at A 3, both caps at once (R = 1024, N * R = 8192), and the A cap at N = 1.
SAMPLE_CASES = ((1, 1, 1, 1), (20, 4, 6, 3), (65, 1, 2, 1), (256, 4, 30, 1))
LOSS_CASES = SAMPLE_CASES + ((64, 4, 30, 3), (1024, 8, 8, 2), (63, 1, 1, 8))
MAX_ROWS, MAX_SAMPLED, MAX_ACTIONS = 1024, 8192, 8


def _f64(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def split(raw):
    """raw [R, 2A] -> (mu raw, log_std raw, mu, tanh(log_std raw)) in float64"""
    raw = _f64(raw)
    A = raw.shape[1] // 2
    return raw[:, :A], raw[:, A:], np.clip(raw[:, :A], -5.0, 5.0), np.tanh(raw[:, A:])


def log_prob(z, mu, th):
    """sum_A log N(z; mu, exp(th)) over the last axis"""
    return (-((z - mu) ** 2) / (2.0 * np.exp(2.0 * th)) - th - HALF_LOG_2PI).sum(-1)


def sample(head_next, head_old, eps):
    """-> dict zn, zt_add, a_next, a_add, each [N, R, A]"""
    eps = _f64(eps)
    _, _, mun, thn = split(head_next)
    _, _, muo, tho = split(head_old)
    zn = mun[None] + np.exp(thn)[None] * eps[0]
    zt = muo[None] + np.exp(tho)[None] * eps[1]
    return dict(zn=zn, zt_add=zt, a_next=np.tanh(zn), a_add=np.tanh(zt))


def loss(head, head_old, q, qt_a, qt_next, qt_add, zt_add, action, reward, done, prob_b, T, mult, eps, gamma, retrace=True):
    """mult = (eta, alpha_mu, alpha_sigma), eps = (eps_eta, eps_alpha_mu, eps_alpha_sigma).  -> dict of float64 values (see the module docstring)."""
    mr, _, mu, th = split(head)
    _, _, mu_o, th_o = split(head_old)
    R, A = mu.shape
    zt = _f64(zt_add)
    N = zt.shape[0]
    q, qt_a, reward, done, prob_b = (_f64(v).reshape(-1) for v in (q, qt_a, reward, done, prob_b))
    qt_next, qt_add = _f64(qt_next).reshape(N, R), _f64(qt_add).reshape(N, R)
    eta, alpha_mu, alpha_sigma = (float(np.float32(v)) for v in mult)
    eps_eta, eps_mu, eps_sigma = (float(np.float32(v)) for v in eps)
    gamma = float(np.float32(gamma))
    ac = np.clip(np.asarray(action, dtype=np.float32).reshape(R, A), np.float32(-ATANH_BOUND), np.float32(ATANH_BOUND)).astype(np.float64)
    z = np.arctanh(ac)
    lp = log_prob(z, mu, th)
    ratio = np.exp(lp) / (prob_b + 1e-6)
    c = np.minimum(ratio, 1.0)
    qret0 = reward + gamma * qt_next.mean(0) * (1.0 - done)
    qret = qret0.copy()
    if retrace and T > 1:
        Q, C, D, QA = qret.reshape(-1, T), c.reshape(-1, T), done.reshape(-1, T), qt_a.reshape(-1, T)
        for t in range(T - 2, -1, -1):
            Q[:, t] += gamma * C[:, t + 1] * (Q[:, t + 1] - QA[:, t + 1]) * (1.0 - D[:, t])
        qret = Q.reshape(-1)
    dq = q - qret
    critic = float((dq ** 2).mean())
    g_q = 2.0 * dq / R
    At = qt_add - qt_add.mean(0, keepdims=True)
    x = At / eta
    xm = x.max(0, keepdims=True)
    e = np.exp(x - xm)
    w = e / e.sum(0, keepdims=True)                                    # [N, R]
    var, var_o = np.exp(2.0 * th), np.exp(2.0 * th_o)
    dm = zt - mu[None]                                                 # [N, R, A]
    lp_add = log_prob(zt, mu[None], th[None])                          # [N, R]
    actor = float(-(w * lp_add).sum(0).mean())
    L = (xm + np.log(e.mean(0, keepdims=True))).reshape(-1)
    eta_loss = eta * eps_eta + eta * float(L.mean())
    wAt = (w * At).sum(0)
    g_eta = eps_eta + float(L.mean()) - float(wAt.mean()) / eta
    d = mu - mu_o
    kld_mu = 0.5 * (d * d * var_o).sum(-1)
    rat = var / var_o
    kld_sigma = 0.5 * (rat.sum(-1) - A + 2.0 * (th_o - th).sum(-1))
    alpha_loss = float((alpha_mu * (eps_mu - kld_mu) + alpha_mu * kld_mu).mean() + (alpha_sigma * (eps_sigma - kld_sigma) + alpha_sigma * kld_sigma).mean())
    g_amu, g_asg = eps_mu - float(kld_mu.mean()), eps_sigma - float(kld_sigma.mean())
    w1, w2 = (w[..., None] * dm).sum(0), (w[..., None] * dm * dm).sum(0)
    g_mu = (-w1 / var + alpha_mu * d * var_o) / R
    g_mu = np.where((mr >= -5.0) & (mr <= 5.0), g_mu, 0.0)
    g_th = (-(w2 / var - 1.0) + alpha_sigma * (rat - 1.0)) / R
    g_head = np.concatenate([g_mu, g_th * (1.0 - th * th)], 1)
    # the multipliers' gradients are DIFFERENCES: an error is measured against the sum of the magnitudes of their terms
    mult_scale = [eps_eta + abs(float(L.mean())) + abs(float(wAt.mean())) / eta, eps_mu + abs(float(kld_mu.mean())),
                  eps_sigma + 0.5 * float((rat.sum(-1) + A + 2.0 * np.abs(th_o - th).sum(-1)).mean())]
    return dict(z=z, log_prob=lp, ratio=ratio, c=c, qret0=qret0, qret=qret, At=At, w=w, kld_mu=kld_mu, kld_sigma=kld_sigma, actor=actor, critic=critic,
                eta_loss=eta_loss, alpha_loss=alpha_loss, grads={"head": g_head, "q": g_q}, mult_grads=[g_eta, g_amu, g_asg], mult_scale=mult_scale,
                extrema=(float(q.min()), float(q.max()), float(At.min()), float(At.max())), mu_raw=mr)


def loss_torch(head, head_old, q, qt_a, qt_next, qt_add, zt_add, action, reward, done, prob_b, T, mult, eps, gamma, retrace=True, dtype=None):
    """mpo.py:199-309 as the reference writes it, from the raw heads and the critic's outputs on, in `dtype` with autograd.  -> the keys of `loss`
    that the acceptance rule compares: the four losses, grads, mult_grads, qret, c."""
    import torch
    from torch.distributions import Normal

    dtype = dtype or torch.float32
    t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)
    head_, q_ = t(head).requires_grad_(True), t(q).reshape(-1, 1).requires_grad_(True)
    R, A = head_.shape[0], head_.shape[1] // 2
    B = R // T
    N = np.asarray(zt_add).shape[0]
    pol = lambda h: (torch.clamp(h[:, :A], min=-5.0, max=5.0), torch.tanh(h[:, A:]).exp())
    mu, std = pol(head_)
    mut, stdt = pol(t(head_old))
    act = t(action).reshape(R, A)
    rew, dn, pb = t(reward).reshape(-1, 1), t(done).reshape(-1, 1), t(prob_b).reshape(-1, 1)
    Qt_a, Qt_next, Qt_add, zt = t(qt_a).reshape(-1, 1), t(qt_next).reshape(N, R, 1), t(qt_add).reshape(N, R, 1), t(zt_add).reshape(N, R, A)
    eta, alpha_mu, alpha_sigma = (torch.tensor(float(np.float32(v)), dtype=dtype, requires_grad=True) for v in mult)
    eps_eta, eps_mu, eps_sigma, gamma = (float(np.float32(v)) for v in (*eps, gamma))
    m = Normal(mu, std)
    z = torch.atanh(torch.clamp(act.float(), -1 + 1e-7, 1 - 1e-7).to(dtype))  # the stored action is a float32 tensor at any `dtype`: the bound rounds as there
    prob = torch.exp(m.log_prob(z).sum(axis=-1, keepdims=True))
    with torch.no_grad():
        c = torch.clip(prob / (pb + 1e-6), max=1.0)
        Qret = rew + gamma * Qt_next.mean(axis=0) * (1 - dn)
        if retrace and T > 1:
            Qret, Qa, cv, dv = (v.view(B, -1, 1) for v in (Qret, Qt_a, c, dn))
            for i in reversed(range(T - 1)):
                Qret[:, i] += gamma * cv[:, i + 1] * (1 - dv[:, i]) * (Qret[:, i + 1] - Qa[:, i + 1])
            Qret = Qret.view(-1, 1)
    log_prob_add = m.log_prob(zt).sum(axis=-1, keepdims=True)
    critic_loss = torch.nn.functional.mse_loss(q_, Qret).mean()
    At = Qt_add - torch.mean(Qt_add, axis=0, keepdims=True)
    w = torch.exp(torch.log_softmax(At / eta, dim=0))
    actor_loss = -torch.mean(torch.sum(w.detach() * log_prob_add, axis=0))
    eta_loss = eta * eps_eta + eta * torch.mean(torch.log(torch.exp(At / eta).mean(axis=0)))
    ss, ss_old = 1.0 / (std ** 2), 1.0 / (stdt ** 2)
    d_mu = mu - mut.detach()
    KLD_mu = 0.5 * torch.sum(d_mu * 1.0 / ss_old.detach() * d_mu, axis=-1)
    mu_loss = torch.mean(alpha_mu * (eps_mu - KLD_mu.detach()) + alpha_mu.detach() * KLD_mu)
    KLD_sigma = 0.5 * (torch.sum(1.0 / ss * ss_old.detach(), axis=-1) - ss.shape[-1] + torch.log(torch.prod(ss, axis=-1) / torch.prod(ss_old.detach(), axis=-1)))
    sigma_loss = torch.mean(alpha_sigma * (eps_sigma - KLD_sigma.detach()) + alpha_sigma.detach() * KLD_sigma)
    alpha_loss = mu_loss + sigma_loss
    (critic_loss + actor_loss + eta_loss + alpha_loss).backward()
    f = lambda v: float(v.detach())
    g = lambda v: float(v.grad) if v.grad is not None else float("nan")
    return dict(actor=f(actor_loss), critic=f(critic_loss), eta_loss=f(eta_loss), alpha_loss=f(alpha_loss), qret=Qret.reshape(-1).numpy().astype(np.float64),
                c=c.reshape(-1).numpy().astype(np.float64), grads={"head": head_.grad.numpy().astype(np.float64), "q": q_.grad.reshape(-1).numpy().astype(np.float64)},
                mult_grads=[g(eta), g(alpha_mu), g(alpha_sigma)])


def sample_torch(head_next, head_old, eps, dtype=None):
    """`sample` in torch at `dtype` (float32: the comparator's own error)."""
    import torch

    dtype = dtype or torch.float32
    t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)
    hn, ho, e = t(head_next), t(head_old), t(eps)
    A = hn.shape[1] // 2
    zn = torch.clamp(hn[:, :A], -5.0, 5.0) + torch.tanh(hn[:, A:]).exp() * e[0]
    zt = torch.clamp(ho[:, :A], -5.0, 5.0) + torch.tanh(ho[:, A:]).exp() * e[1]
    return {k: v.numpy().astype(np.float64) for k, v in dict(zn=zn, zt_add=zt, a_next=torch.tanh(zn), a_add=torch.tanh(zt)).items()}


# ---------------------------------------------------------------------------------------------- kernel cases
def sample_case(R, N, A, seed=0):
    """Raw heads with some mu beyond +-5 (the clamp) and standard normals."""
    rs = np.random.RandomState(1000 * seed + 31 * R + 7 * N + A)
    f = lambda *s: rs.randn(*s).astype(np.float32)
    hn, ho = 1.5 * f(R, 2 * A), 1.5 * f(R, 2 * A)
    hn[0, 0], ho[R // 2, A - 1] = np.float32(6.5), np.float32(-7.25)
    return dict(head_next=hn, head_old=ho, eps=f(2, N, R, A))


VARIANTS = {"plain": 0, "hot": 1, "floor": 2, "alldone": 3}


def case(R, T, N, A, variant="plain", seed=0):
    """Synthetic inputs of one loss-kernel call.  Every case has at least one raw mu of online(s) beyond +-5 (zero gradient there) and, from
    R >= 3 on, stored action components that are exactly +1 and -1 (the atanh clamp); prob_b sits on both sides of the policy's own density, a
    factor of at least 1.5 away from it (c is clipped in some rows and unclipped in others, never near the clip); with T > 1 there is a done
    inside trajectory 0 at T - 2.  Variants: `hot`: eta = 1e-3, where the reference's float32 exp(At / eta) overflows; `floor`: floors just under
    the three multipliers and large first moments, so that each step crosses its floor; `alldone`: every step of trajectory 0 is done."""
    rs = np.random.RandomState(1000 * seed + 97 * R + 13 * T + 5 * N + A + 7919 * VARIANTS[variant])
    f = lambda *s: rs.randn(*s).astype(np.float32)
    head = np.concatenate([1.2 * f(R, A), 0.8 * f(R, A)], 1)
    head[0, 0] = np.float32(6.5)
    if R > 1:
        head[R // 2, A - 1] = np.float32(-7.25)
    head_old = (head + 0.3 * f(R, 2 * A)).astype(np.float32)
    _, _, mu, th = split(head)
    _, _, mu_o, th_o = split(head_old)
    action = np.tanh(mu + 0.3 * np.exp(th) * rs.randn(R, A)).astype(np.float32)  # near the mean: the density of A dimensions stays well above prob_b's 1e-6
    if R >= 3:
        action[1, 0], action[R - 1, A - 1] = np.float32(1.0), np.float32(-1.0)
    zt_add = (mu_o[None] + np.exp(th_o)[None] * rs.randn(N, R, A)).astype(np.float32)
    c = dict(R=R, T=T, N=N, A=A, head=head, head_old=head_old, action=action, zt_add=zt_add, q=2.0 * f(R), qt_next=2.0 * f(N, R), qt_add=2.0 * f(N, R))
    c["qt_a"] = (c["q"] + 0.2 * f(R)).astype(np.float32)
    c["reward"] = rs.choice([-1.0, 0.0, 1.0, 0.5], size=R).astype(np.float32)
    done = (rs.rand(R) < 0.15).astype(np.float32)
    if T > 1:
        done[T - 2] = 1.0  # inside trajectory 0, at the last position the scan's mask reads
        done[0] = 0.0
    if variant == "alldone":
        done[:T] = 1.0
    c["done"] = done
    z = np.arctanh(np.clip(action, np.float32(-ATANH_BOUND), np.float32(ATANH_BOUND)).astype(np.float64))
    dens = np.exp(log_prob(z, mu, th))
    factor = np.where(np.arange(R) % 2 == 0, rs.uniform(0.1, 0.6, R), rs.uniform(1.6, 4.0, R))  # density / prob_b = 1 / factor: even rows clipped
    c["prob_b"] = np.maximum(dens * factor, 1e-30).astype(np.float32)
    c["mult"] = np.asarray([1e-3 if variant == "hot" else 0.7, 0.3, 1.5], np.float32)
    c["m"], c["v"] = np.asarray([0.01, -0.02, 0.03], np.float32), np.asarray([1e-4, 3e-4, 2e-4], np.float32)
    c["floors"] = np.asarray([1e-8, 1e-8, 1e-8], np.float32)
    if variant == "floor":
        c["floors"] = (c["mult"] - np.float32(1e-5)).astype(np.float32)
        c["m"] = np.asarray([0.5, 0.5, 0.5], np.float32)  # a large positive first moment: the step goes down, across the floor
    c["eps"] = (0.1, 0.01, 5e-5)
    c["gamma"] = 0.99
    return c


ARGS = ("head", "head_old", "q", "qt_a", "qt_next", "qt_add", "zt_add", "action", "reward", "done", "prob_b")


def case_args(c):
    return [c[k] for k in ARGS]


def case_truth(c, retrace=True, dtype=None):
    if dtype is None:
        return loss(*case_args(c), c["T"], c["mult"], c["eps"], c["gamma"], retrace)
    return loss_torch(*case_args(c), c["T"], c["mult"], c["eps"], c["gamma"], retrace, dtype)


def distance_from_the_switches(t):
    """How far a truth case stays from the two places where a last-bit difference would change the branch: the c = 1 clip (relative distance of
    the unclipped ratio from 1) and the +-5 clamp of mu (relative distance of |raw mu| from 5).  -> (clip, clamp)"""
    return float(np.abs(t["ratio"] - 1.0).min()), float((np.abs(np.abs(t["mu_raw"]) - 5.0) / 5.0).min())


# ---------------------------------------------------------------------------------------------- replay recipe
COLUMNS = ("state", "action", "reward", "next_state", "done", "prob")


def replay(seed, n, T, S, A, done_rows=()):
    """n stored trajectories of T synthetic transitions, as MPO.interact_callback hands them over: every column [1, T, dim].  Actions are tanh
    of normals with every seventh component exactly +1 or -1 (the atanh clamp); `prob` is log-uniform over four decades, so that
    c = min(prob / prob_b, 1) is clipped in some rows and not in others; done_rows: stored rows whose position T - 2 is an episode end."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        done = rs.rand(1, T, 1) < 0.1
        if i in done_rows and T > 1:
            done[0, T - 2, 0] = True
        action = np.tanh(0.7 * rs.randn(1, T, A)).astype(np.float32)
        flat = action.reshape(-1)
        flat[(i % 7)::7] = np.float32(1.0 if i % 2 else -1.0)
        out.append({"state": rs.randn(1, T, S).astype(np.float32), "action": action, "reward": rs.choice([-1.0, 0.0, 1.0, 0.5], size=(1, T, 1)).astype(np.float32),
                    "next_state": rs.randn(1, T, S).astype(np.float32), "done": done, "prob": np.exp(rs.uniform(np.log(1e-4), 0.0, size=(1, T, 1))).astype(np.float32)})
    return out


# ---------------------------------------------------------------------------------------------- fixtures (tools/gen_golden_mpo_continuous.py)
FIXTURES = ("mpo_cont", "mpo_cont_td", "mpo_cont_pendulum")
NETS = ("actor", "target_actor", "critic", "target_critic")


class Fixture:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN, name + ".npz"))
        h = lambda k: self.z[f"hyper/{k}"]
        self.S, self.A, self.H, self.B, self.T, self.N, self.NS = (int(h(k)) for k in ("S", "A", "H", "B", "T", "N", "NS"))
        self.R = self.B * self.T
        self.lr, self.gamma, self.clip = float(h("lr")), float(h("gamma")), float(h("clip_grad_norm"))
        self.retrace, self.learns, self.recipe, self.thin_limit = bool(int(h("retrace"))), int(h("learns")), bool(int(h("recipe"))), int(h("thin_limit"))
        self.mult = [float(h(k)) for k in NAMES]
        self.floors = [float(h("min_" + k)) for k in NAMES]
        self.eps = [float(h("eps_" + k)) for k in NAMES]
        self.replay_seed, self.np_seed, self.done_rows = int(h("replay_seed")), int(h("np_seed")), tuple(int(v) for v in h("done_rows"))

    def thin(self, a):
        return thin(a, self.thin_limit)

    def agent_kwargs(self):
        kw = dict(state_size=self.S, action_size=self.A, hidden_size=self.H, actor="continuous_policy", critic="continuous_q_network", head="mlp",
                  optim_config={"name": "adam", "lr": self.lr}, buffer_size=max(self.N, 64), batch_size=self.B, start_train_step=0, n_epoch=self.learns,
                  n_step=self.T if self.retrace else 8, clip_grad_norm=self.clip, gamma=self.gamma, run_step=100000, lr_decay=False, num_sample=self.NS,
                  critic_loss_type="retrace" if self.retrace else "1step_TD")
        for j, k in enumerate(NAMES):
            kw[k], kw["min_" + k], kw["eps_" + k] = self.mult[j], self.floors[j], self.eps[j]
        return kw

    def sd0(self, net):
        """The starting weights of one of NETS: stored, or (recipe fixtures) regenerated from the seed."""
        if self.recipe:
            from oracle import synth

            shapes = OrderedDict((k[len(f"shape/{net}/"):], tuple(int(x) for x in self.z[k])) for k in self.z.files if k.startswith(f"shape/{net}/"))
            return recipe_weights(shapes, net, int(self.z["hyper/recipe_seed"]), synth)
        return OrderedDict((k[len(f"sd0/{net}/"):], self.z[k]) for k in self.z.files if k.startswith(f"sd0/{net}/"))

    def replay(self):
        return replay(self.replay_seed, self.N, self.T, self.S, self.A, self.done_rows)

    def learn(self, k):
        """The record of learn k, with the replayed columns of its sampled rows as in_action / in_reward / in_done / in_prob."""
        p = f"l{k}/"
        rec = {key[len(p):]: self.z[key] for key in self.z.files if key.startswith(p)}
        rows = self.replay()
        for key in ("action", "reward", "done", "prob"):
            rec["in_" + key] = np.concatenate([rows[i][key] for i in rec["idx"]], 0).reshape(self.R, -1).astype(np.float32)
        return rec

    def tol(self, key):
        """The GPU tests' tolerance where sums over the samples enter: 2 x the reference's own float32 error against the float64 truth
        (hyper/ref_<key>_err, the largest over the fixture's learns) + 1e-5."""
        return 2.0 * float(self.z[f"hyper/ref_{key}_err"]) + 1e-5


def fixture_truth(fx, rec):
    """`loss` on the reference's own tapped tensors of one learn (every per-row tensor is stored whole in all three fixtures: thinning starts
    above 8192 elements, which only weights and their gradients reach)."""
    head_old = np.concatenate([rec["mut"].astype(np.float64), np.arctanh(np.log(rec["stdt"].astype(np.float64)))], 1)  # mu_old is inside +-5 or ON the bound: the clamp is idempotent
    mult0 = [float(rec[f"mult0/{n}"]) for n in NAMES]
    return loss(rec["head"], head_old, rec["q"], rec["qt_a"], rec["qt_next"], rec["qt_add"], rec["zt_add"], rec["in_action"], rec["in_reward"], rec["in_done"],
                rec["in_prob"], fx.T, mult0, fx.eps, fx.gamma, fx.retrace), mult0


# ---------------------------------------------------------------------------------------------- learning curve
# the reference on the oracle's control env (tools/gen_golden_mpo_continuous.py --only curves): config.mpo.pendulum's settings reduced until three
# seeds run on a CPU
CURVE_CONFIG = dict(S=11, A=3, steps=4000, bin=100, seeds=(1, 2, 3), run_step=4000,
                    agent=dict(state_size=11, action_size=3, hidden_size=128, actor="continuous_policy", critic="continuous_q_network", optim_config={"name": "adam", "lr": 2.5e-4},
                               critic_loss_type="retrace", gamma=0.99, buffer_size=50000, batch_size=32, n_step=4, num_sample=8, start_train_step=500, n_epoch=4,
                               clip_grad_norm=1.0, min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.01, eps_alpha_mu=0.01, eps_alpha_sigma=5e-5, eta=1.0,
                               alpha_mu=1.0, alpha_sigma=1.0, lr_decay=True))


def control_curve(agent, env, steps, bin_):
    """MPO's single-mode loop (act, step, interact_callback, process([window], step)) on a one-env control env with obs() / step(action) ->
    mean reward per step in bins of `bin_` steps."""
    out, acc = [], 0.0
    for step in range(1, steps + 1):
        state = np.array(env.obs(), np.float32)  # the window keeps it for n_step steps
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"], dtype=np.float32).reshape(1, -1))
        tr = {"state": state, "next_state": np.array(nxt, np.float32), "reward": np.asarray(rew, np.float64).reshape(1, 1), "done": np.asarray(done).astype(bool).reshape(1, 1)}
        tr.update(a)
        tr = agent.interact_callback(tr)
        if tr:
            agent.process([tr], step)
        acc += float(np.asarray(rew).reshape(-1)[0])
        if step % bin_ == 0:
            out.append(acc / bin_)
            acc = 0.0
    return out


def curve_tenths(curve):
    """(mean of the first tenth, mean of the last tenth) of a curve given as per-bin means."""
    n = max(1, len(curve) // 10)
    return float(np.mean(curve[:n])), float(np.mean(curve[-n:]))
