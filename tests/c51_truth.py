"""Float64 numpy restatement of the C51 / Rainbow loss (core/agent/rainbow.py:167-239, c51.py:68-109): the ground truth of
tests/test_value_losses_gpu.py.  No torch, no reference.  tests/test_value_losses_cpu.py pins it to the reference's own learn() through the
c51 and rainbow fixtures, so the GPU tests may lean on it at shapes that have no fixture.

With B rows, A actions, K atoms z[k] (the support, float32), n steps, dz = float32((v_max - v_min) / (K - 1)):
  p[b, a, :]  = exp(log_softmax(logit[b, a, :]));  Q[b, a] = sum_k z[k] p[b, a, k]         (the same for next_online and target)
  a*[b]       = first argmax_a Q_sel[b, a], sel = next_online if it is given (rainbow.py:177-181), else target (c51.py:76-80)
  Tz[b, j]    = z[j], then for i = n-1 .. 0:  Tz = reward[b, i] + ((1 - done[b, i]) * gamma) * Tz             (float32, elementwise)
  bb[b, j]    = clip(Tz - v_min, 0, v_max - v_min) / dz;  l = floor(bb), u = ceil(bb);  wl = u - bb, wu = bb - l   (float32, exact)
  term[b, k]  = 1 / K * sum_j ([l_j == k == u_j] + [l_j == k] wl_j + [u_j == k] wu_j)
  non[b, k]   = sum_j tp[b, j] ([l_j == k] wl_j + [u_j == k] wu_j),  tp = p_target[b, a*[b], :]
  m[b, :]     = d0 term + (1 - d0) non,  d0 = done[b, 0];  mass[b] = sum_k m[b, k];  m = m / max(mass, 1e-8)
  KL[b]       = -sum_k m[b, k] log(max(p_act[b, k], 1e-8)),  p_act = p[b, action[b], :];  priority[b] = KL[b] ^ alpha
  loss        = wbar * mean_b KL[b],  wbar = mean_b weights[b] (1 without weights)
  d loss / d logit[b, action[b], k] = (-mt[k] + p_act[k] sum_k' mt[k']) * wbar / B,  mt[k] = m[k] if p_act[k] >= 1e-8 else 0;  zero for the other actions.

What is smooth is float64 (softmaxes, expectations, the projection's sums in ascending source atom j, the normalisation, KL, gradient,
priority, loss).  What decides is float32 on purpose: the Bellman chain, the clip, the division by dz, floor and ceil have no reductions, the
library is built with -ffp-contract=off, and so a kernel has to reproduce l and u bit for bit; wl and wu are exact in float32 (bb and its
neighbouring integers are less than 1 apart) and are widened afterwards.

Quirks of the reference, kept: the terminal branch is keyed on done[:, 0]; an integral bb (l == u) drops its mass in the non-terminal branch
(both weights are 0); the weights enter only through their batch mean ((B, 1) * (B,) broadcasts); the action is clipped to [0, A - 1]; the
greedy next action is the first maximum.

The support is an INPUT (float32 [K]): floor / ceil depend on its last bit, and torch.linspace on the CPU, np.linspace(dtype=float32) and the
kernel's form round it differently (tests/test_value_losses_cpu.py counts the atoms).  default_support restates the form the kernel documents."""
import numpy as np

F32 = np.float32
FLOOR = float(F32(1e-8))  # clamp(min=1e-8) on a float32 tensor

V_MIN, V_MAX, GAMMA, ALPHA = -1.0, 10.0, 0.99, 0.6  # the sweep's hyper-parameters (config.rainbow: v in [-1, 10])


def default_support(v_min, v_max, K):
    """float32 [K]: step = (v_max - v_min) / (K - 1); v_min + step * k below K // 2, v_max - step * (K - 1 - k) from there on."""
    k = np.arange(K)
    step = (F32(v_max) - F32(v_min)) / F32(K - 1)
    lower = F32(v_min) + step * k.astype(F32)
    upper = F32(v_max) - step * (K - 1 - k).astype(F32)
    return np.where(k < K // 2, lower, upper).astype(F32)


def softmax64(x):
    """exp(log_softmax(x)) over the last axis, float64."""
    x = np.asarray(x, dtype=np.float64)
    s = x - x.max(-1, keepdims=True)
    return np.exp(s - np.log(np.exp(s).sum(-1, keepdims=True)))


def bellman_image(support, reward, done, v_min, v_max, gamma):
    """The float32 part.  support float32 [K], reward / done [B, n] -> (l, u int64 [B, K], wl, wu float64 [B, K])."""
    z = np.asarray(support, dtype=F32)
    K = z.size
    r, d = np.asarray(reward, dtype=F32), np.asarray(done, dtype=F32)
    B, n = r.shape
    g, one = F32(gamma), F32(1)
    Tz = np.broadcast_to(z.reshape(1, K), (B, K)).astype(F32)
    for i in reversed(range(n)):
        Tz = r[:, i, None] + ((one - d[:, i, None]) * g) * Tz
    rng = F32(v_max) - F32(v_min)
    dz = F32((float(F32(v_max)) - float(F32(v_min))) / (K - 1))
    bb = np.minimum(np.maximum(Tz - F32(v_min), F32(0)), rng) / dz
    assert bb.dtype == F32
    lf, uf = np.floor(bb), np.ceil(bb)
    wl, wu = uf - bb, bb - lf
    assert wl.dtype == F32 and wu.dtype == F32
    return lf.astype(np.int64), uf.astype(np.int64), wl.astype(np.float64), wu.astype(np.float64)


def c51_truth(logit, next_online, target, action, reward, done, weights, v_min, v_max, gamma, alpha, support=None):
    """logit / next_online (or None) / target [B, A, K]; action [B]; reward / done [B, n] (any shape with B rows); weights [B] or None;
    float32 inputs are taken at their exact values, gamma as the float32 the kernel receives.
    -> dict: kl, prio, mass, clamp_dist, gap, gap_bound, q_best [B]; a_star [B]; grad [B, A, K]; l, u [B, K]; target_dist, p_act [B, K];
       loss, mean_kl, max_Q, max_logit, min_logit; support."""
    z, zt = np.asarray(logit, dtype=np.float64), np.asarray(target, dtype=np.float64)
    B, A, K = z.shape
    sup32 = default_support(v_min, v_max, K) if support is None else np.asarray(support, dtype=F32).reshape(K)
    sup = sup32.astype(np.float64)
    rows = np.arange(B)
    act = np.clip(np.asarray(action, dtype=np.float64).reshape(B).astype(np.int64), 0, A - 1)
    r, d = np.asarray(reward, dtype=F32).reshape(B, -1), np.asarray(done, dtype=F32).reshape(B, -1)
    p = softmax64(z)
    q = (p * sup).sum(-1)
    pt = softmax64(zt)
    q_sel = (pt * sup).sum(-1) if next_online is None else (softmax64(next_online) * sup).sum(-1)
    a_star = q_sel.argmax(-1)  # first maximum
    if A > 1:
        top = np.sort(q_sel, -1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(B, np.inf)
    # what two float32 expectations may be off by: K products and K - 1 additions on probabilities that sum to 1, plus a few ulp of expf / logf
    gap_bound = np.full(B, 2.0 * (K + 8) * 2.0 ** -24 * float(np.abs(sup).max()))
    tp = pt[rows, a_star]
    l, u, wl, wu = bellman_image(sup32, r, d, v_min, v_max, gamma)
    term, non = np.zeros((B, K)), np.zeros((B, K))
    for j in range(K):  # ascending source atom, like the reference's sum over dim 1
        lj, uj = l[:, j], u[:, j]
        np.add.at(term, (rows, lj), (lj == uj).astype(np.float64) + wl[:, j])
        np.add.at(term, (rows, uj), wu[:, j])
        np.add.at(non, (rows, lj), tp[:, j] * wl[:, j])
        np.add.at(non, (rows, uj), tp[:, j] * wu[:, j])
    d0 = d[:, 0].astype(np.float64)[:, None]
    m = d0 * (term / K) + (1.0 - d0) * non
    mass = m.sum(-1)
    m = m / np.maximum(mass, FLOOR)[:, None]
    p_act = p[rows, act]
    kl = -(m * np.log(np.maximum(p_act, FLOOR))).sum(-1)
    wbar = 1.0 if weights is None else float(np.asarray(weights, dtype=np.float64).reshape(B).mean())
    mt = np.where(p_act >= FLOOR, m, 0.0)
    grad = np.zeros_like(z)
    grad[rows, act] = (-mt + p_act * mt.sum(-1, keepdims=True)) * (wbar / B)
    return dict(kl=kl, prio=kl ** alpha, a_star=a_star, gap=gap, gap_bound=gap_bound, q_best=q_sel.max(-1), mass=mass,
                clamp_dist=np.abs(p_act / FLOOR - 1.0).min(-1), grad=grad, l=l, u=u, target_dist=m, p_act=p_act,
                loss=wbar * float(kl.mean()), mean_kl=float(kl.mean()), max_Q=float(q.max()), max_logit=float(z.max()), min_logit=float(z.min()),
                support=sup32)


def near_ties(t):
    """Rows whose two best selector Q lie closer than float32 can tell apart (rows with gap == 0 included)."""
    return t["gap"] <= np.maximum(t["gap_bound"], 1e-5 * (1.0 + np.abs(t["q_best"])))


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_value_losses_gpu.py (inputs only; the CPU suite proves the conditions on every case before a GPU sees them).
# Every B of {1, 3, 63, 64, 65, 127, 128, 129, 200, 1024, 1025, 1027, 1030} (<= 1024: one workgroup per sample, whose weight preload has the
# pieces lane < B, lane + 64 < B and a tail from lane + 128; above: one wave per sample, ragged last block unless B % 4 == 0), every A of
# {1, 2, 3, 4, 5, 8, 9, 18} (actions stride over 4 waves, zero rows over 3), every K of {2, 51, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256}
# (one to four atoms per lane), every n_step of {0, 1, 3, 64, 65} (above 64 the block kernel loads rewards directly) and every flag
# combination at least once; every B >= 129 with weights.
FLAGS = ("none", "double", "per", "double+per")
SWEEP = [
    # (B, A, K, n_step, flags, variant)
    (1, 1, 2, 0, "none", "plain"),
    (3, 2, 192, 1, "double+per", "outside"),  # the shape at which the float32 oracle's own support moves one atom's l / u
    (3, 18, 256, 3, "double", "plain"),
    (63, 3, 63, 1, "per", "plain"),
    (64, 4, 64, 3, "double+per", "plain"),
    (65, 5, 65, 3, "none", "terminal_first"),
    (127, 8, 127, 1, "double", "plain"),
    (128, 9, 128, 3, "per", "plain"),
    (129, 2, 129, 3, "double+per", "on_atoms"),
    (129, 4, 51, 64, "per", "plain"),
    (200, 3, 193, 65, "double+per", "plain"),
    (200, 5, 51, 3, "per", "clamped_p"),
    (1024, 2, 51, 3, "double+per", "plain"),
    (1024, 1, 255, 1, "per", "plain"),
    (1024, 3, 63, 3, "per", "terminal_first"),
    (1025, 2, 51, 3, "double+per", "plain"),
    (1025, 5, 65, 1, "per", "all_done"),
    (1025, 3, 51, 1, "double", "exact_tie"),
    (1027, 3, 64, 3, "per", "terminal_first"),
    (1027, 9, 2, 1, "double", "plain"),
    (1030, 4, 51, 3, "double+per", "action_clip"),
    (1030, 2, 65, 3, "per", "on_atoms"),
    (3, 2, 51, 3, "double", "exact_tie"),
    (65, 3, 129, 1, "double+per", "exact_tie"),
    (64, 8, 51, 65, "double", "plain"),
    (3, 4, 255, 64, "none", "plain"),
    (63, 18, 51, 3, "none", "action_clip"),
    (1, 9, 193, 1, "per", "plain"),
    (128, 5, 256, 0, "double", "clamped_p"),
    (200, 1, 192, 3, "per", "outside"),
    (127, 2, 2, 3, "per", "all_done"),
    (65, 4, 128, 3, "double", "outside"),
]
# Seeds chosen so that no row of a case sits on a discontinuity (tests/test_value_losses_cpu.py counts them): with seed 0 these four have
# one row each whose two best selector Q are closer than 1e-5 (1 + |Q|).  (3, 2, 192, 1): a seed whose rewards put one atom's Bellman image
# between the kernel's support and np.linspace's, so that the float32 oracle on its own support takes another l / u there.
SEEDS = {(3, 2, 192, 1, "double+per", "outside"): 10,
         (1024, 3, 63, 3, "per", "terminal_first"): 1, (1027, 3, 64, 3, "per", "terminal_first"): 1, (1030, 4, 51, 3, "double+per", "action_clip"): 1,
         (128, 5, 256, 0, "double", "clamped_p"): 1}
BLOCK_VS_WAVE = (1025, 2, 51, 3, "double+per", "plain")  # run whole (wave per sample) and as its first 1024 rows (workgroup per sample)


def case_id(c):
    return "B{}-A{}-K{}-n{}-{}-{}".format(*c)


def sweep_case(B, A, K, n_step, flags, variant, seed=None):
    """Seeded float32 inputs: logits ~ N(0, 1); rewards from {-1, 0, 0.5, 1} (over long windows mostly 0, so that the n-step return stays
    on the support); done with probability 0.3 per step (0.5 / n per step over long windows).
    -> dict(logit, next_online | None, target [B, A, K]; action [B]; reward, done [B, max(n_step, 1)]; weights [B] | None; n_step)."""
    assert flags in FLAGS
    seed = SEEDS.get((B, A, K, n_step, flags, variant), 0) if seed is None else seed
    rs = np.random.RandomState((1000003 * seed + 7919 * B + 131 * A + 17 * K + 3 * n_step + FLAGS.index(flags)) % (2 ** 31))
    n = max(n_step, 1)
    z, zn, zt = (rs.randn(B, A, K).astype(F32) for _ in range(3))
    action = rs.randint(0, A, size=B).astype(F32)
    reward = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], dtype=F32), size=(B, n))
    if n > 3:
        reward = np.where(rs.rand(B, n) < 3.0 / n, reward, F32(0)).astype(F32)
    done = (rs.rand(B, n) < (0.3 if n <= 3 else 0.5 / n)).astype(F32)
    weights = (0.1 + 0.9 * rs.rand(B)).astype(F32)
    dz = (V_MAX - V_MIN) / (K - 1)
    if variant == "all_done":
        done[:] = 1.0
    elif variant == "terminal_first":
        done[::2, 0] = 1.0
    elif variant == "outside":  # |r| = 20: Tz leaves [v_min, v_max], bb sits on a clamped end, l == u
        far = rs.rand(B, n) < 0.2
        reward[far] = rs.choice(np.array([-20.0, 20.0], dtype=F32), size=int(far.sum()))
        for b, r0 in ((0, 20.0), (1, -20.0)):  # not terminal and out of reach for good: every atom's mass is dropped
            if b < B:
                reward[b], done[b] = 0.0, 0.0
                reward[b, 0] = r0
    elif variant == "on_atoms":  # rewards on v_min + k dz; dz = 11 / (K - 1) has to be exact in float32: K in {65, 129}
        assert F32(dz) == dz and K > 4
        for b in range(0, B, 2):  # terminal: the whole distribution lands on one interior atom
            done[b, 0] = 1.0
            reward[b, 0] = V_MIN + rs.randint(1, K - 1) * dz
        if n > 1:
            for b in range(1, B, 4):  # not terminal, cut after the first step: every atom lands on one interior atom and is dropped
                done[b, 0], done[b, 1] = 0.0, 1.0
                reward[b, 0], reward[b, 1] = V_MIN + rs.randint(1, K - 1) * dz, 0.0
    elif variant == "clamped_p":  # the taken action's atoms in three groups e^40 apart: the lower two fall under the 1e-8 clamp
        assert K >= 3
        for b in range(0, B, 2):
            shift = rs.choice(np.array([-40.0, 0.0, 40.0], dtype=F32), size=K)
            shift[:3] = (-40.0, 0.0, 40.0)
            z[b, int(action[b])] += shift
    elif variant == "exact_tie":  # the selector's best row twice, bit for bit: the first of the two must win
        assert A > 1 and "double" in flags
        qn = (softmax64(zn) * default_support(V_MIN, V_MAX, K).astype(np.float64)).sum(-1)
        for b in range(0, B, 2):
            a1 = int(qn[b].argmax())
            zn[b, (a1 + 1 + (b // 2) % (A - 1)) % A] = zn[b, a1]  # a copy before or after the original
    elif variant == "action_clip":
        action[0] = -1.0
        action[1::7] = A + 2.0
        action[2::11] = -1.0
    else:
        assert variant == "plain", variant
    return dict(logit=z, next_online=zn if "double" in flags else None, target=zt, action=action, reward=reward, done=done,
                weights=weights if "per" in flags else None, n_step=n_step)


def truth_of(case):
    d = {k: v for k, v in case.items() if k != "n_step"}
    return c51_truth(v_min=V_MIN, v_max=V_MAX, gamma=GAMMA, alpha=ALPHA, **d)
