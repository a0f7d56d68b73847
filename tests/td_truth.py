"""Float64 numpy restatement of the five TD losses behind jh_td_loss (dqn.py:128-141, double.py:28-39, multistep.py:41-50, per.py:54-74,
ape_x.py:96-116): the ground truth of tests/test_value_losses_gpu.py.  No torch, no reference.  tests/test_value_losses_cpu.py pins it to
the reference's own learn() through the dqn, double, multistep, per and ape_x fixtures.

With B rows and A actions, q = Q(s)[b, action[b]] (the action clipped to [0, A - 1]):
  boot[b] = Qt(s')[b, a*[b]], a*[b] = first argmax_a Q(s')[b, a]   with the online net's Q(s') (double);   max_a Qt(s')[b, a] without
  y[b]    = r + (1 - d) * gamma * boot                              plain          (dqn.py:135-137)
            r + boot * (gamma * (1 - d))                            double         (double.py:35-37, per.py:62-64)
            y = boot; for i = n-1 .. 0: y = r_i + (1 - d_i) * gamma * y            n_step > 0, with either boot (multistep.py:47-48, ape_x.py:105-106)
  td[b]   = |y - q|
  Huber (no weights):  loss = mean_b smooth_l1(q - y), beta = 1;     d loss / d q = clamp(q - y, -1, 1) / B;   priority = td
  PER (weights w):     loss = mean_b w td^2;                         d loss / d q = 2 w (q - y) / B;           priority = td ^ alpha
  the gradient goes to the taken action only;  stats = (loss, max_b q, mean_b td).
Everything is float64 on the float32 inputs' exact values (gamma as the float32 the kernel receives); the operation order of each target form
is the reference's, although in float64 it no longer matters."""
import numpy as np

F32 = np.float32
GAMMA, ALPHA = 0.99, 0.6


def td_truth(q, q_next_online, q_next_target, action, reward, done, weights, gamma, alpha, n_step=0):
    """q / q_next_online (or None) / q_next_target [B, A]; action [B]; reward / done [B, max(n_step, 1)] (any shape with B rows); weights [B] or None.
    -> dict: grad [B, A]; prio, td, y, kink_dist (||q - y| - 1|, where Huber changes branch), gap, gap_bound (the double-Q selection's two
       best values and what their comparison may be off by: nothing, they are inputs) [B]; a_star [B] (None without double); loss, max_Q, mean_td."""
    qa = np.asarray(q, dtype=np.float64)
    B, A = qa.shape
    qnt = np.asarray(q_next_target, dtype=np.float64)
    rows = np.arange(B)
    act = np.clip(np.asarray(action, dtype=np.float64).reshape(B).astype(np.int64), 0, A - 1)
    n = max(int(n_step), 1)
    r, d = np.asarray(reward, dtype=np.float64).reshape(B, n), np.asarray(done, dtype=np.float64).reshape(B, n)
    g = float(F32(gamma))
    gap, a_star = np.full(B, np.inf), None
    if q_next_online is not None:
        qno = np.asarray(q_next_online, dtype=np.float64)
        a_star = qno.argmax(-1)  # first maximum
        boot = qnt[rows, a_star]
        if A > 1:
            top = np.sort(qno, -1)
            gap = top[:, -1] - top[:, -2]
    else:
        boot = qnt.max(-1)
    if n_step > 0:
        y = boot
        for i in reversed(range(n)):
            y = r[:, i] + (1.0 - d[:, i]) * g * y
    elif q_next_online is not None:
        y = r[:, 0] + boot * (g * (1.0 - d[:, 0]))
    else:
        y = r[:, 0] + (1.0 - d[:, 0]) * g * boot
    qt = qa[rows, act]
    diff = qt - y
    td = np.abs(y - qt)
    if weights is None:
        ad = np.abs(diff)
        loss = float(np.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5).mean())
        gq = np.clip(diff, -1.0, 1.0) / B
        prio = td
    else:
        w = np.asarray(weights, dtype=np.float64).reshape(B)
        loss = float((w * td * td).mean())
        gq = 2.0 * w * diff / B
        prio = td ** alpha
    grad = np.zeros_like(qa)
    grad[rows, act] = gq
    return dict(grad=grad, prio=prio, td=td, y=y, kink_dist=np.abs(td - 1.0), gap=gap, gap_bound=np.zeros(B), a_star=a_star, q_best=boot,
                loss=loss, max_Q=float(qt.max()), mean_td=float(td.mean()))


def near_ties(t, q_next_online):
    """Rows of a double-Q case whose two best Q(s') lie closer than 1e-5 (1 + |Q|): none may (the kernel compares the inputs themselves, so
    only an exact tie could go either way, and the first maximum is the rule there)."""
    if q_next_online is None:
        return np.zeros(t["gap"].shape, bool)
    best = np.abs(np.asarray(q_next_online, dtype=np.float64)).max(-1)
    return t["gap"] <= np.maximum(t["gap_bound"], 1e-5 * (1.0 + best))


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_value_losses_gpu.py.  Every B of {1, 255, 256, 257, 513} (one lane per row, 256 rows per block: one block, a full
# one, one row into the second, a third block), every A of {1, 2, 6, 18}, all four flag combinations x n_step of {0, 1, 3}.
FLAGS = ("none", "double", "per", "double+per")
SWEEP = [
    # (B, A, n_step, flags, variant)
    (1, 1, 0, "none", "plain"),
    (255, 2, 1, "none", "plain"),
    (256, 6, 3, "none", "plain"),
    (257, 18, 0, "double", "plain"),
    (513, 2, 1, "double", "plain"),
    (1, 6, 3, "double", "plain"),
    (255, 18, 0, "per", "plain"),
    (256, 1, 1, "per", "plain"),
    (257, 2, 3, "per", "plain"),
    (513, 6, 0, "double+per", "plain"),
    (255, 6, 1, "double+per", "plain"),
    (256, 18, 3, "double+per", "plain"),
    (257, 6, 0, "none", "zero_td"),
    (513, 18, 0, "double+per", "zero_td"),
    (257, 6, 3, "double+per", "action_clip"),
    (255, 2, 0, "none", "action_clip"),
]


def case_id(c):
    return "B{}-A{}-n{}-{}-{}".format(*c)


def sweep_case(B, A, n_step, flags, variant, seed=0):
    """Seeded float32 inputs: Q(s) ~ 2 N(0, 1), both Q(s') ~ N(0, 1) (|q - y| on both sides of 1), rewards ~ N(0, 1), done with probability
    0.2 per step.  -> dict(q, q_next_online | None, q_next_target [B, A]; action [B]; reward, done [B, max(n_step, 1)]; weights [B] | None; n_step)."""
    assert flags in FLAGS
    rs = np.random.RandomState((1000003 * seed + 7919 * B + 131 * A + 3 * n_step + FLAGS.index(flags)) % (2 ** 31))
    n = max(n_step, 1)
    q = (2.0 * rs.randn(B, A)).astype(F32)
    qno, qnt = rs.randn(B, A).astype(F32), rs.randn(B, A).astype(F32)
    action = rs.randint(0, A, size=B).astype(F32)
    reward = rs.randn(B, n).astype(F32)
    done = (rs.rand(B, n) < 0.2).astype(F32)
    weights = (0.1 + 0.9 * rs.rand(B)).astype(F32)
    if variant == "zero_td":  # terminal rows whose taken Q equals the reward: y = r exactly in every target form, td = 0
        assert n_step == 0
        for b in range(0, B, 3):
            done[b, 0] = 1.0
            q[b, int(action[b])] = reward[b, 0]
    elif variant == "action_clip":
        action[0] = -1.0
        action[1::7] = A + 2.0
        action[2::11] = -1.0
    else:
        assert variant == "plain", variant
    return dict(q=q, q_next_online=qno if "double" in flags else None, q_next_target=qnt, action=action, reward=reward, done=done,
                weights=weights if "per" in flags else None, n_step=n_step)


def truth_of(case):
    return td_truth(gamma=GAMMA, alpha=ALPHA, **case)
