"""The discrete SAC's two loss kernels (csrc/jh_sac_discrete.hip) restated in plain numpy, float64 by default (dtype=np.float32: the restatement
whose distance from float64 bounds what a float32 evaluation may lose), and the case table of tests/test_sac_discrete_gpu.py."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)  # torch.distributions clamps float32 probabilities to [eps, 1 - eps] before the log
FIXTURES = ("sac_discrete", "sac_discrete_static", "sac_discrete_cartpole")
NETS = ("actor", "critic1", "target_critic1", "critic2", "target_critic2")  # the reference's construction order (sac.py:75-95)


def categorical(z, dtype=np.float64):
    """-> (p, clamped log p, the clamp does not bind, entropy [B]) of softmax(z) as Categorical(probs).entropy() forms them."""
    z = np.asarray(z).astype(dtype)
    zm = z.max(1, keepdims=True)
    lp = (z - zm) - np.log(np.exp(z - zm).sum(1, keepdims=True))
    lo, hi = dtype(np.log(EPS)), dtype(np.log1p(-EPS))
    lc = np.clip(lp, lo, hi)
    p = np.exp(lp)
    return p, lc, (lp >= lo) & (lp <= hi), -(p * lc).sum(1)


def critic_loss(la_next, qt1, qt2, q1, q2, action, reward, done, gamma, alpha, dtype=np.float64):
    """sac.py:193-217 -> dict(y, loss [2], max_Q, grad [2, B, A], next_q [2, B], H)."""
    p, _, _, H = categorical(la_next, dtype)
    nq = np.stack([(p * np.asarray(q).astype(dtype)).sum(1) for q in (qt1, qt2)])
    r, d = (np.asarray(v).astype(dtype).reshape(-1) for v in (reward, done))
    y = r + (1 - d) * dtype(gamma) * (np.minimum(nq[0], nq[1]) + dtype(alpha) * H)
    B, A = p.shape
    rows, a = np.arange(B), np.clip(np.asarray(action).reshape(-1).astype(np.int64), 0, A - 1)
    grad, loss = np.zeros((2, B, A), dtype), []
    for i, q in enumerate((q1, q2)):
        e = np.asarray(q).astype(dtype)[rows, a] - y
        grad[i, rows, a] = 2 * e / B
        loss.append((e * e).mean())
    return dict(y=y, loss=np.asarray(loss), max_Q=y.max(), grad=grad, next_q=nq, H=H)


def actor_loss(la, q1, q2, alpha, log_alpha, target_entropy, dtype=np.float64):
    """sac.py:235-255 -> dict(actor_loss, alpha_loss, mean_Q, entropy, alpha (refreshed), grad [B, A] to the raw logits, g_log_alpha, q [2, B])."""
    p, lc, free, H = categorical(la, dtype)
    Q = [np.asarray(q).astype(dtype) for q in (q1, q2)]
    e = np.stack([(p * q).sum(1) for q in Q])
    w1 = np.where(e[0] < e[1], 1.0, np.where(e[1] < e[0], 0.0, 0.5)).astype(dtype)[:, None]  # torch.min's backward
    g = -dtype(alpha) * (lc + free) + w1 * Q[0] + (1 - w1) * Q[1]
    grad = -(p * (g - (p * g).sum(1, keepdims=True))) / p.shape[0]
    mn = np.minimum(e[0], e[1])
    g_la = H.mean() - dtype(target_entropy)
    return dict(actor_loss=-(dtype(alpha) * H + mn).mean(), alpha_loss=dtype(log_alpha) * g_la, mean_Q=mn.mean(), entropy=H.mean(),
                alpha=np.exp(dtype(log_alpha)), grad=grad, g_log_alpha=g_la, q=e)


def adam_scalar(x, grad, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step number t on one scalar -> (x, m, v)."""
    m, v = m + (grad - m) * (1 - b1), v * b2 + (1 - b2) * grad * grad
    return x - lr / (1 - b1 ** t) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)), m, v


# ---------------------------------------------------------------------------------------------- the GPU cases
# A in {2, 3, 5, 64}: lane groups of 2, 4, 8, 64 (A = 3, 5 pad lanes inside the group).  Per A, B = 1, one group short of a wave, a batch that ends inside a
# workgroup, the first batch that needs a second workgroup (256 / G rows + 1), 1024 (at A = 64 a wave IS one group: no batch is one group short of it).
# mode: "static", or "dyn<k>": dynamic alpha with k Adam steps of log_alpha behind it.  Every case with B >= 2 has done rows, a last row whose logits push all
# probabilities but one under float32 eps by a wide margin (both ends of the clamp bind), |Q| from 1e-3 to 1e3 across rows and both orders of q1 / q2.
# "tie": row 0 has q1 == q2 exactly, from DIFFERENT Q rows (case_inputs), so d(logits) of that row depends on the tie's weights.
# "near": EVERY row has two equal leading logits and all other probabilities 3 to 30 times under eps, at |Q| = 1e-4: the clamped log and its zeroed derivative
# are 9 % and 6 % of those lanes' d(logits) entries.  A probability under eps moves an output by less than float32 resolves next to the row's other terms, so
# the float32 gap of these cases is large and the gap rule cannot see the clamp; the GPU test adds an entrywise bound for them (the kernel works in double).
# gap: the largest distance of the float32 restatement from float64 over every output (distance() below), checked by tests/test_sac_discrete_cpu.py.
CASES = [
    dict(A=2, B=1, mode="static", gap=1.972e-7), dict(A=2, B=31, mode="dyn0", gap=2.506e-7), dict(A=2, B=100, mode="dyn1", gap=2.310e-7),
    dict(A=2, B=129, mode="static", tie=True, gap=2.021e-7), dict(A=2, B=1024, mode="dyn0", gap=2.253e-7),
    dict(A=3, B=1, mode="dyn1", gap=9.546e-8), dict(A=3, B=15, mode="static", gap=2.094e-7), dict(A=3, B=50, mode="dyn0", tie=True, gap=4.308e-7),
    dict(A=3, B=65, mode="dyn1", gap=8.481e-7), dict(A=3, B=1024, mode="static", gap=1.219e-7), dict(A=3, B=15, mode="dyn0", near=True, gap=7.084e-5),
    dict(A=5, B=1, mode="dyn0", gap=1.430e-7), dict(A=5, B=7, mode="dyn1", gap=7.878e-7), dict(A=5, B=20, mode="static", gap=7.012e-7),
    dict(A=5, B=33, mode="dyn0", gap=1.543e-7), dict(A=5, B=1024, mode="dyn1", tie=True, gap=9.682e-8),
    dict(A=64, B=1, mode="static", gap=2.946e-7), dict(A=64, B=3, mode="dyn0", gap=1.119e-7), dict(A=64, B=5, mode="dyn1", tie=True, gap=1.328e-7),
    dict(A=64, B=1024, mode="dyn0", gap=1.407e-7), dict(A=64, B=5, mode="static", near=True, gap=2.843e-4),
]
GAMMA, ALPHA, LOG_ALPHA, ALPHA_LR, PRIOR_M, PRIOR_V = 0.99, 0.37, -0.8, 5e-2, 0.02, 3e-4


def case_id(c):
    return f"A{c['A']}-B{c['B']}-{c['mode']}" + "".join("-" + k for k in ("tie", "near") if c.get(k))


def case_inputs(c):
    """float32 inputs of both kernels: la_next, qt1, qt2, q1, q2 (critic), la, q1_pi, q2_pi (actor), action, reward, done."""
    A, B = c["A"], c["B"]
    rng = np.random.RandomState(1000 * A + B)
    scale = 10.0 ** rng.uniform(-3, 3, (B, 1)) if not c.get("near") else 1e-4
    x = {k: (rng.randn(B, A) * scale).astype(np.float32) for k in ("qt1", "qt2", "q1", "q2", "q1_pi", "q2_pi")}
    x.update({k: (1.5 * rng.randn(B, A)).astype(np.float32) for k in ("la_next", "la")})
    x["action"] = rng.randint(0, A, B).astype(np.float32)
    x["reward"] = rng.choice([-1.0, 0.0, 1.0, 0.5], B).astype(np.float32)
    x["done"] = (rng.rand(B) < 0.25).astype(np.float32)
    rows = np.arange(B)
    for k in ("la_next", "la"):
        if c.get("near"):  # log p of the small lanes = logit - log 2: log eps - 3.4 .. log eps - 1.2
            x[k][:] = (-16.5 - 2.0 * rng.rand(B, A)).astype(np.float32)
            x[k][rows, rows % A], x[k][rows, (rows + 1) % A] = 0.0, 0.0
        elif B >= 2:
            x[k][B - 1] = -40.0
            x[k][B - 1, (B - 1) % A] = 0.0
    if B >= 2:
        x["done"][0], x["done"][1] = 1.0, 0.0
    if c.get("tie"):  # equal probabilities on actions 0 and 1, the Q rows (a, b, 0 ...) and (b, a, 0 ...): p a + p b == p b + p a in any order of summation
        for la, qa, qb in (("la", "q1_pi", "q2_pi"), ("la_next", "qt1", "qt2")):
            x[la][0, :2], x[qa][0], x[qb][0] = 2.0, 0.0, 0.0
            x[qa][0, :2], x[qb][0, :2] = (768.0, -320.0), (-320.0, 768.0)
    return x


def case_truth(c, dtype=np.float64):
    """Both kernels and the temperature's step on case c -> ({name: everything the kernels write}, log_alpha's steps before, critic dict, actor dict)."""
    x = case_inputs(c)
    alpha, la = float(np.float32(ALPHA)), float(np.float32(LOG_ALPHA))
    te = float(np.float32(-np.log(1 / c["A"]) * 0.98))
    cr = critic_loss(x["la_next"], x["qt1"], x["qt2"], x["q1"], x["q2"], x["action"], x["reward"], x["done"], GAMMA, alpha, dtype)
    ac = actor_loss(x["la"], x["q1_pi"], x["q2_pi"], alpha, la, te, dtype)
    k = {"static": None, "dyn0": 0, "dyn1": 1}[c["mode"]]
    m, v = (float(np.float32(PRIOR_M)), float(np.float32(PRIOR_V))) if k else (0.0, 0.0)
    la1 = la if k is None else float(adam_scalar(dtype(la), ac["g_log_alpha"], dtype(m), dtype(v), k + 1, dtype(np.float32(ALPHA_LR)))[0])
    out = {"dQ1": cr["grad"][0], "dQ2": cr["grad"][1], "d logits": ac["grad"], "critic_loss1": cr["loss"][0], "critic_loss2": cr["loss"][1], "max_Q": cr["max_Q"]}
    out.update({n: ac[n] for n in ("actor_loss", "alpha_loss", "mean_Q", "alpha", "entropy")}, log_alpha=la1)
    return out, k, cr, ac


def distance(got, want):
    """(the largest, over the outputs, of max |difference| / max |entry|, that output's name)."""
    f = lambda a: np.asarray(a, np.float64)
    return max((float(np.abs(f(got[n]) - f(w)).max() / max(np.abs(f(w)).max(), 1e-300)), n) for n, w in want.items())
