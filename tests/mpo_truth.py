"""Float64 numpy statement of jh_mpo_loss_discrete's contract (include/jorldy_hip.h; core/agent/mpo.py:312-386 and 416-419 for a discrete policy):
the comparator of tests/test_mpo_cpu.py and tests/test_mpo_gpu.py (test infrastructure, not the product).  Inputs are float32 arrays; everything
after them is float64.

  loss               c, Qret before and after the Retrace scan, At, the E-step weights, the four losses, d(loss)/d(actor logits of s), d(loss)/d(q of s),
                     the gradients of eta and alpha_mu (alpha_sigma has none for a discrete policy) and the extrema of q and At
  multiplier_step    one Adam step (torch.optim.Adam's single-tensor arithmetic) of one scalar in float64, then max(x, floor) with a NaN kept
  loss_torch         the SAME quantities the way the reference writes them -- log(softmax), exp(At / eta) without the row maximum -- with torch
                     autograd in a given dtype: float32 is the comparator whose own error against float64 the acceptance rule of the GPU tests
                     needs (tests/test_vmpo_gpu.py's `_scalar`, fp64_truth.grad_vs_exact), float64 cross-checks `loss`
and the case builders of the kernel tests, the replay recipe and the reader of the fixtures of tools/gen_golden_mpo.py."""
import os
from collections import OrderedDict

import numpy as np

NAMES = ("eta", "alpha_mu", "alpha_sigma")
STATS = ("actor_loss", "critic_loss", "eta_loss", "alpha_loss", "eta", "alpha_mu", "alpha_sigma", "min_Q", "max_Q", "min_At", "max_At")
NETS = ("actor", "target_actor", "critic", "target_critic")
COLUMNS = ("state", "action", "reward", "next_state", "done", "prob")
FIXTURES = ("mpo_discrete", "mpo_td", "mpo_cartpole")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# the kernel tests' optimizer block
LR, BETAS, ADAM_EPS, STEP0 = 3e-3, (0.9, 0.999), 1e-8, 4
# (B, T, A): R = 3, 20, 128, 264, 1024, 1 -- less than one wavefront, a wavefront multiple, ragged over several wavefronts, the cap, a single row
KERNEL_CASES = ((3, 1, 2), (5, 4, 3), (16, 8, 2), (33, 8, 6), (128, 8, 18), (1, 1, 2))
# the reference on the oracle's CartPole (tools/gen_golden_mpo.py --only curves): config.mpo.cartpole reduced until three seeds run on a CPU
CURVE_CONFIG = dict(steps=4000, seeds=(1, 2, 3), run_step=4000,
                    agent=dict(state_size=4, action_size=2, hidden_size=128, actor="discrete_policy", critic="discrete_q_network", optim_config={"name": "adam", "lr": 2.5e-4},
                               critic_loss_type="retrace", gamma=0.99, buffer_size=50000, batch_size=32, n_step=4, start_train_step=500, n_epoch=4, clip_grad_norm=1.0,
                               min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.02, eps_alpha_mu=0.01, eps_alpha_sigma=0.01, eta=1.0, alpha_mu=1.0,
                               alpha_sigma=1.0, lr_decay=True))


def _lsm(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))


def loss(la, la_next, la_old, q, qt, qt_next, action, reward, done, prob_b, T, mult, eps, gamma, retrace=True):
    """The six network outputs [R, A], the replayed columns [R], T rows per trajectory (row b * T + t), mult = (eta, alpha_mu, alpha_sigma),
    eps = (eps_eta, eps_alpha_mu).  -> dict of float64 values (see the module docstring)."""
    la, la_next, la_old, q, qt, qt_next = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (la, la_next, la_old, q, qt, qt_next))
    R, A = la.shape
    a = np.clip(np.asarray(action).reshape(-1).astype(np.int64), 0, A - 1)
    reward, done, prob_b = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(-1) for v in (reward, done, prob_b))
    eta, alpha_mu = float(np.float32(mult[0])), float(np.float32(mult[1]))
    eps_eta, eps_mu = float(np.float32(eps[0])), float(np.float32(eps[1]))
    gamma = float(np.float32(gamma))
    rows = np.arange(R)
    lp, lpn, lpo = _lsm(la), _lsm(la_next), _lsm(la_old)
    pi, pin, pio = np.exp(lp), np.exp(lpn), np.exp(lpo)
    c = np.minimum(pi[rows, a] / (prob_b + 1e-6), 1.0)
    qret0 = reward + gamma * (pin * qt_next).sum(-1) * (1.0 - done)
    qret = qret0.copy()
    if retrace and T > 1:
        Q, C, D, QA = qret.reshape(-1, T), c.reshape(-1, T), done.reshape(-1, T), qt[rows, a].reshape(-1, T)
        for t in range(T - 2, -1, -1):
            Q[:, t] += gamma * C[:, t + 1] * (Q[:, t + 1] - QA[:, t + 1]) * (1.0 - D[:, t])
        qret = Q.reshape(-1)
    dq = q[rows, a] - qret
    critic = float((dq ** 2).mean())
    g_q = np.zeros((R, A))
    g_q[rows, a] = 2.0 * dq / R
    V = (pio * qt).sum(-1, keepdims=True)
    At = qt - V
    x = At / eta
    xm = x.max(-1, keepdims=True)
    e = np.exp(x - xm)
    w = e / e.sum(-1, keepdims=True)
    actor = float(-(w * lp).sum(-1).mean())
    su = (pio * e).sum(-1, keepdims=True)
    L = (xm + np.log(su)).reshape(-1)
    u = pio * e / su
    eta_loss = eta * eps_eta + eta * float(L.mean())
    uAt = (u * At).sum(-1)
    g_eta = eps_eta + float(L.mean()) - float(uAt.mean()) / eta
    kld = (pio * (lpo - lp)).sum(-1)
    alpha_loss = float((alpha_mu * (eps_mu - kld) + alpha_mu * kld).mean())
    g_mu = eps_mu - float(kld.mean())
    g_la = ((pi - w) + alpha_mu * (pi - pio)) / R
    # the multipliers' gradients are DIFFERENCES: an error is measured against the sum of the magnitudes of their terms
    mult_scale = [eps_eta + abs(float(L.mean())) + abs(float(uAt.mean())) / eta, eps_mu + abs(float(kld.mean()))]
    return dict(c=c, qret0=qret0, qret=qret, At=At, w=w, kld=kld, actor=actor, critic=critic, eta_loss=eta_loss, alpha_loss=alpha_loss,
                grads={"la": g_la, "q": g_q}, mult_grads=[g_eta, g_mu, None], mult_scale=mult_scale,
                extrema=(float(q.min()), float(q.max()), float(At.min()), float(At.max())))


def multiplier_step(x, grad, m, v, step, lr, floor, betas=(0.9, 0.999), eps=1e-8):
    """ONE Adam step of one scalar in float64 from the given optimizer state (`step` steps taken so far; torch.optim.Adam's single-tensor
    arithmetic: m and v updated, bias corrections, denom = sqrt(v) / sqrt(bc2) + eps), then max(x, floor) as torch.max does it (a NaN stays).
    -> (x, m, v) as Python floats."""
    x, grad, m, v, lr, floor = (float(t) for t in (x, grad, m, v, lr, floor))
    b1, b2 = float(betas[0]), float(betas[1])
    t = step + 1
    m = m + (grad - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * grad * grad
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps
    x = x - step_size * (m / denom)
    x = floor if x < floor else x
    return float(x), float(m), float(v)


def loss_torch(la, la_next, la_old, q, qt, qt_next, action, reward, done, prob_b, T, mult, eps, gamma, retrace=True, dtype=None):
    """mpo.py:312-386 as the reference writes it, from the logits and q-values on, in `dtype` with autograd.  -> the keys of `loss` that the
    acceptance rule compares: the four losses, grads, mult_grads, qret."""
    import torch

    dtype = dtype or torch.float32
    t = lambda v: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype)
    la_, q_ = t(la).requires_grad_(True), t(q).requires_grad_(True)
    R, A = la_.shape
    B = R // T
    pi, pi_next, pit = (torch.exp(torch.log_softmax(v, dim=-1)) for v in (la_, t(la_next), t(la_old)))
    Qt, Qt_next = t(qt), t(qt_next)
    act = torch.as_tensor(np.clip(np.asarray(action).reshape(-1, 1).astype(np.int64), 0, A - 1))
    rew, dn, pb = t(reward).reshape(-1, 1), t(done).reshape(-1, 1), t(prob_b).reshape(-1, 1)
    eta = torch.tensor(float(np.float32(mult[0])), dtype=dtype, requires_grad=True)
    alpha_mu = torch.tensor(float(np.float32(mult[1])), dtype=dtype, requires_grad=True)
    eps_eta, eps_mu, gamma = float(np.float32(eps[0])), float(np.float32(eps[1])), float(np.float32(gamma))
    Q_a = q_.gather(1, act)
    with torch.no_grad():
        Qt_a = Qt.gather(1, act)
        c = torch.clip(pi.gather(1, act) / (pb + 1e-6), max=1.0)
        Qret = rew + gamma * torch.sum(pi_next * Qt_next, axis=-1, keepdim=True) * (1 - dn)
        if retrace and T > 1:
            Qret, Qt_a, c, dn = (v.view(B, -1, 1) for v in (Qret, Qt_a, c, dn))
            for i in reversed(range(T - 1)):
                Qret[:, i] += gamma * c[:, i + 1] * (Qret[:, i + 1] - Qt_a[:, i + 1]) * (1 - dn[:, i])
            Qret = Qret.view(-1, 1)
    critic_loss = torch.nn.functional.mse_loss(Q_a, Qret).mean()
    Vt = torch.sum(pit * Qt, axis=-1, keepdims=True)
    At = Qt - Vt
    w = torch.exp(torch.log_softmax(At / eta, dim=-1))
    actor_loss = -torch.mean(torch.sum(w.detach() * torch.log(pi), axis=-1))
    eta_loss = eta * eps_eta + eta * torch.mean(torch.log(torch.sum(pit * torch.exp(At / eta), axis=-1)))
    KLD = torch.sum(pit * (torch.log(pit) - torch.log(pi)), axis=-1)
    alpha_loss = torch.mean(alpha_mu * (eps_mu - KLD.detach()) + alpha_mu.detach() * KLD)
    (critic_loss + actor_loss + eta_loss + alpha_loss).backward()
    f = lambda v: float(v.detach())
    return dict(actor=f(actor_loss), critic=f(critic_loss), eta_loss=f(eta_loss), alpha_loss=f(alpha_loss), qret=Qret.reshape(-1).numpy().astype(np.float64),
                grads={"la": la_.grad.numpy().astype(np.float64), "q": q_.grad.numpy().astype(np.float64)},
                mult_grads=[float(eta.grad) if eta.grad is not None else float("nan"), float(alpha_mu.grad), None])


# ---------------------------------------------------------------------------------------------- kernel cases
def case(B, T, A, variant="plain", seed=0):
    """Synthetic inputs of one kernel call.  Variants: `plain`; `hot`: eta = 1e-3, where the reference's float32 exp(At / eta) overflows;
    `floor`: floors just under the multipliers so that the step of each crosses its floor.  Every case with T > 1 has done = 1 inside a
    trajectory (at T - 2 of trajectory 0 when there is one) and prob_b on both sides of the clip."""
    rs = np.random.RandomState(1000 * seed + 97 * B + 13 * T + A + {"plain": 0, "hot": 1, "floor": 2}[variant])
    R = B * T
    f = lambda *s: rs.randn(*s).astype(np.float32)
    c = dict(B=B, T=T, A=A, la=f(R, A), q=2.0 * f(R, A), qt_next=2.0 * f(R, A))
    c["la_next"] = f(R, A)
    c["la_old"] = (c["la"] + 0.3 * f(R, A)).astype(np.float32)
    c["qt"] = (c["q"] + 0.2 * f(R, A)).astype(np.float32)
    c["action"] = rs.randint(0, A, size=R).astype(np.float32)
    c["reward"] = rs.choice([-1.0, 0.0, 1.0, 0.5], size=R).astype(np.float32)
    done = (rs.rand(R) < 0.15).astype(np.float32)
    if T > 1:
        done[T - 2] = 1.0  # inside trajectory 0, at the last position the scan's mask reads
        done[0] = 0.0
    c["done"] = done
    pb = rs.uniform(0.02, 1.0, size=R).astype(np.float32)
    pb[::2] = np.float32(0.02)  # pi[a] / 0.02 > 1 for any pi[a] > 0.02: clipped; the others mostly are not
    pb[1::4] = np.float32(0.999)
    c["prob_b"] = pb
    c["mult"] = np.asarray([1e-3 if variant == "hot" else 0.7, 0.3, 1.5], np.float32)
    c["m"], c["v"] = np.asarray([0.01, -0.02, 0.0], np.float32), np.asarray([1e-4, 3e-4, 0.0], np.float32)
    c["floors"] = np.asarray([1e-8, 1e-8, 1e-8], np.float32)
    if variant == "floor":
        c["floors"] = np.asarray([c["mult"][0] - 1e-5, c["mult"][1] - 1e-5, 1e-8], np.float32)
        c["m"] = np.asarray([0.5, 0.5, 0.0], np.float32)  # a large positive first moment: the step goes down, across the floor
    c["eps"] = (0.02, 0.01)
    c["gamma"] = 0.99
    return c


def case_args(c):
    return [c[k] for k in ("la", "la_next", "la_old", "q", "qt", "qt_next", "action", "reward", "done", "prob_b")]


def case_truth(c, retrace=True, dtype=None):
    if dtype is None:
        return loss(*case_args(c), c["T"], c["mult"], c["eps"], c["gamma"], retrace)
    return loss_torch(*case_args(c), c["T"], c["mult"], c["eps"], c["gamma"], retrace, dtype)


# ---------------------------------------------------------------------------------------------- replay recipe and fixtures
def replay(seed, N, T, S, A, done_rows=()):
    """N stored trajectories of T synthetic transitions, as MPO.interact_callback hands them over: every column [1, T, dim].  `prob` is drawn
    on both sides of the policy's probabilities (so that c = min(pi / prob, 1) is clipped in some rows and not in others); done_rows: stored
    rows whose position T - 2 is an episode end."""
    rs = np.random.RandomState(seed)
    out = []
    for n in range(N):
        done = rs.rand(1, T, 1) < 0.1
        if n in done_rows and T > 1:
            done[0, T - 2, 0] = True
        out.append({"state": rs.randn(1, T, S).astype(np.float32), "action": rs.randint(0, A, size=(1, T, 1)),
                    "reward": rs.choice([-1.0, 0.0, 1.0, 0.5], size=(1, T, 1)).astype(np.float32), "next_state": rs.randn(1, T, S).astype(np.float32),
                    "done": done, "prob": rs.uniform(0.05, 1.0, size=(1, T, 1)).astype(np.float32)})
    return out


def thin(a, limit, stride=61):
    a = np.asarray(a)
    return a if (not limit or a.size <= limit) else np.ascontiguousarray(a.reshape(-1)[::stride])


class Fixture:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN, name + ".npz"))
        h = lambda k: self.z[f"hyper/{k}"]
        self.S, self.A, self.H, self.B, self.T, self.N = (int(h(k)) for k in ("S", "A", "H", "B", "T", "N"))
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
        kw = dict(state_size=self.S, action_size=self.A, hidden_size=self.H, actor="discrete_policy", critic="discrete_q_network", head="mlp",
                  optim_config={"name": "adam", "lr": self.lr}, buffer_size=max(self.N, 64), batch_size=self.B, start_train_step=0, n_epoch=self.learns,
                  n_step=self.T, clip_grad_norm=self.clip, gamma=self.gamma, run_step=100000, lr_decay=False,
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
        p = f"l{k}/"
        return {key[len(p):]: self.z[key] for key in self.z.files if key.startswith(p)}


def recipe_weights(shapes, net, seed, synth):
    """Recipe weights of one of the four nets (oracle/synth.py's streams, keyed by name: the net's own prefix keeps the four apart); the
    policy's last layer is scaled down as ppo_recipe scales policy heads."""
    sd = synth.recipe_state_dict([(f"{net}.{k}", s) for k, s in shapes.items()], seed)
    out = OrderedDict((k[len(net) + 1:], v) for k, v in sd.items())
    for k in out:
        if k.startswith("pi.") and out[k].ndim == 2:
            out[k] = np.ascontiguousarray(out[k] * np.float32(0.3), dtype=np.float32)
    return out


def load_fixture(name):
    return Fixture(name)


def curve_tenths(curve):
    """(mean of the first tenth, mean of the last tenth) of a per-step reward curve given as per-bin means."""
    n = max(1, len(curve) // 10)
    return float(np.mean(curve[:n])), float(np.mean(curve[-n:]))
