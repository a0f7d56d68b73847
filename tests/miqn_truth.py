"""Restatement of Munchausen IQN's target and loss (core/agent/m_iqn.py:29-95, agent/utils.py:29-39) with torch autograd on the CPU: the
ground truth of the M-IQN tests.  float64 is the truth; the same function in float32 is the torch-CPU comparator of fp64_truth's
criterion.  tests/test_miqn_cpu.py pins it to the reference's own learn() through the three fixtures (tools/gen_golden_miqn.py), so the
GPU tests may lean on it at shapes that have no fixture.  The network is iqn_truth.iqn_forward.  No reference code is read.

Per sample b, with z1 = online(state) under the first draw tau_1, z4 = online(state) under a fresh draw, zt = target(next_state),
all [N, A]; x = mean_n z4, x' = mean_n zt, a = action, tau_e the entropy temperature, every exp behind a subtracted row maximum:
  lp       = x[a] - (max x + tau_e log sum_k exp((x_k - max x) / tau_e))                 log_policy
  pi       = exp(log_softmax((x' - max x') / tau_e)),  logpi = x' - (max x' + tau_e log sum_k exp((x'_k - max x') / tau_e))
  T[j]     = reward + alpha * clip(lp, l_0, 0) + (1 - done) * gamma * sum_k pi_k (zt[j, k] - logpi_k)          theta_target
  e[j, i]  = T[j] - z1[i, a],  loss = 1 / (B N) sum_{b, j, i} (1 - tau_1[b, i] if e < 0 else tau_1[b, i]) * smooth_l1(e)
Statistics: max_Q = max mean_n z1, max_logit / min_logit = the extremes of z4 (m_iqn.py:50 gives the name `logit` to z4)."""
import numpy as np
import torch

from iqn_truth import KEYS, NET_SHAPES, SWEEP_SHAPES, iqn_forward  # noqa: F401  (the network and the shapes are IQN's)


def miqn_loss(logit, logit_again, target, action, reward, done, tau, gamma, alpha, tau_e, l_0, dtype=torch.float64):
    """Inputs as arrays or tensors ([B, N, A] x 3, [B] x 3, tau float32 [B, N]); float32 inputs are taken at their exact values.  When
    `logit` is a tensor with a graph, the loss is attached to it (backward through a network); otherwise d loss / d logit is returned.
    Actions are clamped into [0, A).
    -> dict(loss_t (tensor), loss, grad [B, N, A] | None, theta_target [B, N], log_policy [B], clipped [B] bool (lp < l_0), max_Q,
            max_logit, min_logit, abs_e_min, abs_e_max), numpy in `dtype`."""
    c = lambda v: v.to(dtype) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)).to(dtype)
    attached = torch.is_tensor(logit) and logit.requires_grad
    z = logit if attached else c(logit).clone().requires_grad_(True)
    z4, zt = c(logit_again).detach(), c(target).detach()
    B, N, A = z.shape
    act = torch.as_tensor(np.asarray(action, dtype=np.float64).reshape(B)).long().clamp(0, A - 1)
    r, d = c(reward).reshape(B, 1), c(done).reshape(B, 1)
    tau32 = torch.as_tensor(np.asarray(tau, dtype=np.float32).reshape(B, N))
    inv_tau = (1 - tau32).to(dtype)  # the reference forms 1 - tau in float32
    tau_t = tau32.to(dtype)
    rows = torch.arange(B)
    means = lambda v: v.transpose(1, 2).contiguous().mean(-1)  # [B, A], in the reference's memory order (logits2Q)

    def scaled_log_softmax(x):
        mx = x.max(-1, keepdim=True)[0]
        return x - (mx + tau_e * torch.log(torch.exp((x - mx) / tau_e).sum(-1, keepdim=True)))

    with torch.no_grad():
        x, xn = means(z4), means(zt)
        lp = scaled_log_softmax(x)[rows, act].reshape(B, 1)
        mun = alpha * torch.clip(lp, min=l_0, max=0)
        logpi = scaled_log_softmax(xn)
        pi = torch.exp(torch.log_softmax((xn - xn.max(-1, keepdim=True)[0]) / tau_e, -1))
        soft = (pi.unsqueeze(2) * (zt.transpose(1, 2) - logpi.unsqueeze(2))).sum(1)  # [B, N] (j)
        T = r + mun + (1 - d) * gamma * soft
    P = z[rows, :, act]  # [B, N] (i)
    e = T[:, :, None] - P[:, None, :]  # [B, j, i]
    hub = torch.nn.functional.smooth_l1_loss(*torch.broadcast_tensors(P[:, None, :], T[:, :, None]), reduction="none")
    wgt = torch.where(e < 0, inv_tau[:, None, :], tau_t[:, None, :])
    loss = (wgt * hub).sum(2).mean()
    grad = None
    if not attached:
        loss.backward()
        grad = z.grad.numpy()
    ae = e.detach().abs()
    n = lambda t: t.detach().numpy()
    return dict(loss_t=loss, loss=float(loss.detach()), grad=grad, theta_target=n(T), log_policy=n(lp).reshape(B), clipped=n(lp < l_0).reshape(B),
                max_Q=float(means(z.detach()).max()), max_logit=float(z4.max()), min_logit=float(z4.min()), abs_e_min=float(ae.min()), abs_e_max=float(ae.max()))


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_miqn_gpu.py (inputs only; the CPU suite checks its properties before a GPU sees them).
HYPER = dict(gamma=0.99, alpha=0.9, tau_e=0.03, l_0=-1.0)
VARIANTS = ("plain", "all_done", "large", "wide", "flat", "tau1")
SWEEP = [(B, A, N, v) for (B, A, N) in SWEEP_SHAPES for v in VARIANTS]
# at these `plain` cases at least one row lies on each side of the log-policy clip and pairs lie on each side of the Huber knee
BOTH_SIDES = [(7, 5, 33), (32, 2, 64), (255, 6, 51)]


def sweep_case(B, A, N, variant, seed=0):
    """Seeded float32 inputs: logits = a level per (row, action) ~ N(0, 1) + noise per sample ~ N(0, 1) -- the quantile means, which
    carry the policies, spread like M-DQN's sweep's q values whatever N is --, rewards from {-1, 0, 0.5, 1}, about 10 % done,
    tau ~ U(0, 1) per (row, sample).  `all_done`: done = 1 on every row; `large`: logits x 0.05 and reward 5, so that |e| > 1 for every
    pair; `wide`: logits x 20 (one-hot policies, exp underflows, the clip is active); `flat`: logits x 0.01 (|log_policy| << |l_0|: no
    row clips); `tau1`: tau_e = 1.
    -> (dict of arrays logit, logit_again, target [B, N, A]; action, reward, done [B]; tau [B, N]), hyper dict."""
    rs = np.random.RandomState(1000003 * seed + 7919 * B + 131 * A + N + 29)
    z, z4, zt = ((rs.randn(B, 1, A) + rs.randn(B, N, A)).astype(np.float32) for _ in range(3))
    action = rs.randint(0, A, size=B).astype(np.float32)
    reward = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32), size=B)
    done = (rs.rand(B) < 0.1).astype(np.float32)
    tau = rs.rand(B, N).astype(np.float32)
    hyper = dict(HYPER)
    if variant == "all_done":
        done[:] = 1.0
    scale = {"large": 0.05, "wide": 20.0, "flat": 0.01}.get(variant)
    if scale is not None:
        z, z4, zt = (np.float32(scale) * v for v in (z, z4, zt))
    if variant == "large":
        reward[:] = 5.0
    if variant == "tau1":
        hyper["tau_e"] = 1.0
    return dict(logit=z, logit_again=z4, target=zt, action=action, reward=reward, done=done, tau=tau), hyper
