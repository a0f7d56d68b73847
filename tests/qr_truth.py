"""Float64 numpy restatement of QR-DQN's loss (core/agent/qrdqn.py:60-95): the ground truth of the QR-DQN tests.  No torch, no reference.
tests/test_qrdqn_cpu.py pins it to the reference's own learn() through the three fixtures, so the GPU tests may lean on it at shapes
that have no fixture.

With B rows, A actions, N quantiles:  P[b, i] = logit[b, action[b], i];  a*[b] = first argmax_a mean_i next_online[b, a, i];
T[b, j] = reward[b] + (1 - done[b]) * gamma * target[b, a*[b], j];  e[b, j, i] = T[b, j] - P[b, i];
loss = 1 / (B N) * sum_{b, j, i} (1 - tau[i] if e < 0 else tau[i]) * smooth_l1(e);
d loss / d logit[b, action[b], i] = -1 / (B N) * sum_j w[b, j, i] * clamp(e[b, j, i], -1, 1), zero for the other actions."""
import numpy as np


def qr_truth(logit, next_online, target, action, reward, done, tau, gamma, a_star=None):
    """All inputs as arrays ([B, A, N] x 3, [B] x 3, [N]); float32 inputs are taken at their exact values.
    a_star: use these next actions instead of the float64 argmax (to score a kernel's loss on rows where the selection is a near-tie).
    -> dict(loss, grad [B, A, N], a_star [B], max_Q, max_logit, min_logit, row_loss [B], gap [B], gap_bound [B])."""
    z, zn, zt = (np.asarray(v, dtype=np.float64) for v in (logit, next_online, target))
    B, A, N = z.shape
    act = np.clip(np.asarray(action, dtype=np.float64).reshape(B).astype(np.int64), 0, A - 1)
    r, d = np.asarray(reward, dtype=np.float64).reshape(B), np.asarray(done, dtype=np.float64).reshape(B)
    tau = np.asarray(tau, dtype=np.float32).reshape(N)
    inv_tau = (np.float32(1) - tau).astype(np.float64)  # the reference forms 1 - tau in float32 (qrdqn.py:31)
    tau = tau.astype(np.float64)
    rows = np.arange(B)
    q, qn = z.mean(-1), zn.mean(-1)
    best = qn.argmax(-1)  # first maximum
    sel = best if a_star is None else np.asarray(a_star, dtype=np.int64).reshape(B)
    P = z[rows, act]  # [B, N] (i)
    T = r[:, None] + (1.0 - d[:, None]) * gamma * zt[rows, sel]  # [B, N] (j)
    e = T[:, :, None] - P[:, None, :]  # [B, j, i]
    ae = np.abs(e)
    hub = np.where(ae < 1.0, 0.5 * e * e, ae - 0.5)
    w = np.where(e < 0.0, inv_tau[None, None, :], tau[None, None, :])
    row_loss = (w * hub).sum((1, 2)) / N
    grad = np.zeros_like(z)
    grad[rows, act] = -(w * np.clip(e, -1.0, 1.0)).sum(1) / (B * N)
    # how far apart the two best quantile means of online(s') are, and what two fp32 sums of N terms may be off by
    if A > 1:
        top = np.sort(qn, -1)
        gap = top[:, -1] - top[:, -2]
    else:
        gap = np.full(B, np.inf)
    gap_bound = 2.0 * N * 2.0 ** -24 * np.abs(zn).reshape(B, -1).max(-1)
    return dict(loss=float(row_loss.sum() / B), grad=grad, a_star=best, max_Q=float(q.max()), max_logit=float(z.max()), min_logit=float(z.min()),
                row_loss=row_loss, gap=gap, gap_bound=gap_bound)


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_qrdqn_gpu.py (inputs only; the CPU suite checks the near-tie count of every case before a GPU sees them).
# Every B of {1, 3, 32, 255, 512, 1030}, every A of {1, 2, 6, 18}, every N of {1, 8, 51, 64, 65, 200, 256} at least once.
SWEEP = [
    # (B, A, N, variant)
    (1, 1, 1, "plain"),
    (3, 2, 8, "plain"),
    (32, 18, 200, "plain"),
    (512, 6, 200, "plain"),
    (255, 6, 51, "plain"),
    (1030, 2, 64, "plain"),
    (32, 6, 65, "plain"),
    (3, 18, 256, "plain"),
    (255, 1, 256, "plain"),
    (1, 6, 200, "plain"),
    (32, 2, 200, "all_done"),  # done = 1 on every row: T[b, :] = reward[b]
    (32, 6, 51, "ties"),       # T == P exactly for some pairs: e == 0 takes the tau branch and contributes 0
]


def sweep_case(B, A, N, variant, seed=0):
    """Seeded float32 inputs: logits ~ N(0, 1) (e = T - P then has a spread of about 1.4 around the reward: |e| on both sides of 1),
    rewards from {-1, 0, 0.5, 1}, about 10 % done.  -> dict of arrays (logit, next_online, target [B, A, N]; action, reward, done [B])."""
    rs = np.random.RandomState(1000003 * seed + 7919 * B + 131 * A + N)
    z, zn, zt = (rs.randn(B, A, N).astype(np.float32) for _ in range(3))
    action = rs.randint(0, A, size=B).astype(np.float32)
    reward = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32), size=B)
    done = (rs.rand(B) < 0.1).astype(np.float32)
    if variant == "all_done":
        done[:] = 1.0
    if variant == "ties":
        done[::2] = 1.0  # T[b, j] = reward[b] + 0 * ... = reward[b] exactly on these rows
        for b in range(0, B, 2):
            z[b, int(action[b]), ::3] = reward[b]  # ... and so is every third prediction quantile
    return dict(logit=z, next_online=zn, target=zt, action=action, reward=reward, done=done)
