"""Restatement of Rainbow-IQN (core/network/rainbow_iqn.py:9-113, core/agent/rainbow_iqn.py:158-243) with torch autograd on the CPU: the
ground truth of the Rainbow-IQN tests, written on tests/iqn_truth.py's functions plus the noisy dueling tail.  float64 is the truth; the same
functions in float32 are the torch-CPU comparator of fp64_truth's criterion.  tests/test_riqn_cpu.py pins them to the reference's own
learn() through the three fixtures (tools/gen_golden_riqn.py), so the GPU tests may lean on them at shapes that have no fixture.  No
reference code is read.

Network: IQN's trunk up to h = relu(l2(relu(l1(psi * phi)))) [R, N, H] (iqn_truth.iqn_forward with the identity in q's place), then
  x_a = relu(h W_a1 + b_a1), x_v = relu(h W_v1 + b_v1), x_a = x_a W_a2 + b_a2 [R, N, A], x_v = x_v W_v2 + b_v2 [R, N, 1],
  out = x_a - mean_a x_a + x_v,   W = mu_w + sig_w * eps_w ([in, out]), b = mu_b + sig_b * eps_b.
One noise set is a forward's draws in draw order (a1, v1, a2, v2), flattened:
  factorized   per layer eps_i [in], eps_j [out]: eps_w = outer(f(eps_i), f(eps_j)), eps_b = f(eps_j), f(e) = sign(e) sqrt|e|
  independent  per layer eps_w [in, out], eps_b [out]
None: eps = 0 (is_train False).  The draws are float32 values; f and the products are formed in `dtype`.
Loss, with P[b, i] = logit[b, i, action[b]], a*[b] = first argmax_a mean_n next_online[b, n, a], T[b, j] = target[b, j, a*[b]] folded as
T = reward[b, k] + (1 - done[b, k]) * gamma * T for k = n_step - 1 .. 0, e[b, j, i] = T[b, j] - P[b, i]:
  loss_b = 1 / N * sum_{j, i} (1 - tau[b, i] if e < 0 else tau[b, i]) * smooth_l1(e),  prio_b = loss_b ^ alpha,
  loss = mean over [B, B] of weights[:, None] * loss_b[None, :] = mean(w) * mean(loss_b): the reference multiplies weights [B, 1] with
  loss [B] (rainbow_iqn.py:217-219), the broadcast Rainbow's categorical loss has too."""
import numpy as np
import torch

import iqn_truth as I

NOISY_KEYS = tuple(f"{p}_{t}" for t in ("a1", "v1", "a2", "v2") for p in ("mu_w", "sig_w", "mu_b", "sig_b"))
TRUNK_KEYS = I.KEYS[:10]
KEYS = NOISY_KEYS + TRUNK_KEYS  # the reference module's state_dict order: its own parameters first, the submodules' after


def layer_dims(H, A):
    return (("a1", H, H), ("v1", H, H), ("a2", H, A), ("v2", H, 1))


def noise_len(H, A, noise_type):
    return sum((i * o + o) if noise_type == "independent" else (i + o) for _, i, o in layer_dims(H, A))


def split_noise(flat, H, A, noise_type):
    """One flat noise set -> {tag: (first draw, second draw)}: (eps_i [in], eps_j [out]) or (eps_w [in, out], eps_b [out]), float32 arrays --
    the injection format of the agents' `_noise` hook (NativeNet.pack_noise)."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    assert flat.size == noise_len(H, A, noise_type)
    out, o = {}, 0
    for tag, i, j in layer_dims(H, A):
        n0 = i * j if noise_type == "independent" else i
        first = flat[o : o + n0].reshape((i, j) if noise_type == "independent" else (i,))
        out[tag] = (first, flat[o + n0 : o + n0 + j])
        o += n0 + j
    return out


def _eps(pair, noise_type, dtype):
    a, b = (torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype) for v in pair)
    if noise_type == "independent":
        return a, b
    f = lambda e: torch.sign(e) * torch.sqrt(torch.abs(e))
    return torch.outer(f(a), f(b)), f(b)


def riqn_forward(sd, x, tau, noise=None, noise_type="factorized", dtype=torch.float64):
    """sd: {state_dict key: tensor} (used as they are when they already have `dtype`, so that leaves with requires_grad stay leaves); x [R, S];
    tau float32 [R, N]; noise: one flat noise set, a split_noise dict, or None.  -> logits [R, N, A] in `dtype`, with the graph attached."""
    w = {k: (v if torch.is_tensor(v) and v.dtype == dtype else torch.as_tensor(np.asarray(v)).to(dtype)) for k, v in sd.items()}
    H, A = w["mu_w_a2"].shape
    trunk = {k: w[k] for k in TRUNK_KEYS}
    trunk["q.weight"], trunk["q.bias"] = torch.eye(H, dtype=dtype), torch.zeros(H, dtype=dtype)  # x * 1 + 0 sums: h itself, exactly
    h = I.iqn_forward(trunk, x, tau, dtype)
    if noise is not None and not isinstance(noise, dict):
        noise = split_noise(noise, H, A, noise_type)

    def noisy(t, tag):
        W, b = w[f"mu_w_{tag}"], w[f"mu_b_{tag}"]
        if noise is not None:
            ew, eb = _eps(noise[tag], noise_type, dtype)
            W, b = W + w[f"sig_w_{tag}"] * ew, b + w[f"sig_b_{tag}"] * eb
        return torch.matmul(t, W) + b

    x_a = noisy(torch.relu(noisy(h, "a1")), "a2")
    x_v = noisy(torch.relu(noisy(h, "v1")), "v2")
    return x_a - x_a.mean(dim=2, keepdim=True) + x_v


def riqn_loss(logit, next_online, target, action, reward, done, weights, tau, gamma, alpha, dtype=torch.float64, a_star=None):
    """Inputs as arrays or tensors ([B, N, A] x 3, action [B], reward / done [B, n_step], weights [B], tau float32 [B, N]); float32 inputs are
    taken at their exact values.  When `logit` is a tensor with a graph, the loss is attached to it; otherwise d loss / d logit is returned.
    a_star: use these next actions instead of the argmax.
    -> dict(loss_t, loss, loss_b [B], prio [B], grad [B, N, A] | None, a_star [B], theta_target [B, N], max_Q, max_logit, min_logit, gap [B],
            gap_bound [B], kink [B]: the smallest distance of a row's |e| from 0 and from 1)."""
    c = lambda v: v.to(dtype) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)).to(dtype)
    attached = torch.is_tensor(logit) and logit.requires_grad
    z = logit if attached else c(logit).clone().requires_grad_(True)
    zn, zt = c(next_online).detach(), c(target).detach()
    B, N, A = z.shape
    act = torch.as_tensor(np.asarray(action, dtype=np.float64).reshape(B)).long().clamp(0, A - 1)
    r, d = c(reward).reshape(B, -1), c(done).reshape(B, -1)
    w = c(weights).reshape(B)
    tau32 = torch.as_tensor(np.asarray(tau, dtype=np.float32).reshape(B, N))
    inv_tau = (1 - tau32).to(dtype)  # the reference forms 1 - tau in float32 (rainbow_iqn.py:204)
    tau_t = tau32.to(dtype)
    rows = torch.arange(B)
    qn = zn.mean(1)
    best = qn.argmax(-1)  # first maximum
    sel = best if a_star is None else torch.as_tensor(np.asarray(a_star)).long().reshape(B)
    P = z[rows, :, act]  # [B, N] (i)
    T = zt[rows, :, sel]  # [B, N] (j)
    for k in reversed(range(r.shape[1])):
        T = r[:, k : k + 1] + (1 - d[:, k : k + 1]) * gamma * T
    e = T[:, :, None] - P[:, None, :]  # [B, j, i]
    hub = torch.nn.functional.smooth_l1_loss(*torch.broadcast_tensors(P[:, None, :], T[:, :, None]), reduction="none")
    wgt = torch.where(e < 0, inv_tau[:, None, :], tau_t[:, None, :])
    loss_b = (wgt * hub).sum(2).mean(1)
    loss = (w.reshape(B, 1) * loss_b).mean()  # [B, B]
    grad = None
    if not attached:
        loss.backward()
        grad = z.grad.numpy()
    zd = z.detach()
    if A > 1:
        top = torch.sort(qn.double(), -1)[0]
        gap = (top[:, -1] - top[:, -2]).numpy()
    else:
        gap = np.full(B, np.inf)
    gap_bound = 2.0 * N * 2.0 ** -24 * zn.double().abs().reshape(B, -1).max(-1)[0].numpy()
    ae = e.detach().double().abs().reshape(B, -1)
    kink = torch.minimum(ae.min(1)[0], (ae - 1).abs().min(1)[0]).numpy()
    lb = loss_b.detach()
    return dict(loss_t=loss, loss=float(loss.detach()), loss_b=lb.numpy(), prio=torch.pow(lb, alpha).numpy(), grad=grad, a_star=best.numpy(), theta_target=T.detach().numpy(),
                max_Q=float(zd.mean(1).max()), max_logit=float(zd.max()), min_logit=float(zd.min()), gap=gap, gap_bound=gap_bound, kink=kink)


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_riqn_gpu.py (inputs only; tests/test_riqn_cpu.py checks its properties before a GPU sees them).
SWEEP_B, SWEEP_A, SWEEP_N, SWEEP_STEPS = (1, 3, 257), (2, 5, 64), (1, 63, 64, 65, 256), (1, 2, 5)
SWEEP = [(B, A, N, n) for B in SWEEP_B for A in SWEEP_A for N in SWEEP_N for n in SWEEP_STEPS]
SWEEP_GAMMA, SWEEP_ALPHA = 0.5, 0.6
KINK = 2.0 ** -20
MAX_SEEDS = 16


def _sweep_draw(B, A, N, n_step, seed):
    rs = np.random.RandomState(1000003 * seed + 7919 * B + 131 * A + 17 * N + n_step)
    # the taken quantiles, the target quantiles and the rewards sit on dyadic grids and gamma is 1/2: every product and sum of the fold and
    # every e = T - P is exact in float32 and in float64, and e is an odd multiple of 2^-9 -- at least 2^-9 from the kinks at 0 and +-1
    z = (rs.randint(-12, 13, size=(B, N, A)) / 4.0 + 2.0 ** -9).astype(np.float32)
    zt = (rs.randint(-12, 13, size=(B, N, A)) / 4.0).astype(np.float32)
    zn = rs.randn(B, N, A).astype(np.float32)  # the selector: continuous, so that two means are never exactly equal
    action = rs.randint(0, A, size=B).astype(np.float32)
    reward = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32), size=(B, n_step))
    done = (rs.rand(B, n_step) < 0.15).astype(np.float32)
    for b in range(min(B, n_step)):  # a done at every window position, alone in its window (B >= n_step), and a window without one
        done[b] = 0.0
        done[b, b] = 1.0
    if B > n_step:
        done[n_step] = 0.0
    weights = (0.1 + 0.9 * rs.rand(B)).astype(np.float32)
    weights[rs.randint(0, B)] = 1.0  # the batch's largest weight is 1 (per_buffer.py:94)
    tau = rs.rand(B, N).astype(np.float32)
    return dict(logit=z, next_online=zn, target=zt, action=action, reward=reward, done=done, weights=weights, tau=tau)


def selection_gaps(next_online):
    z = np.asarray(next_online, dtype=np.float64)
    B, N, A = z.shape
    top = np.sort(z.mean(1), -1)
    return top[:, -1] - top[:, -2], 2.0 * N * 2.0 ** -24 * np.abs(z).reshape(B, -1).max(-1)


def sweep_case(B, A, N, n_step):
    """Seeded float32 inputs of one sweep case, the first seed of 0 .. MAX_SEEDS - 1 whose selector has no near-tie row (the truth alone
    decides: two fp32 sums of N terms can be off by gap_bound).  -> (dict of arrays, seed)."""
    for seed in range(MAX_SEEDS):
        d = _sweep_draw(B, A, N, n_step, seed)
        gap, bound = selection_gaps(d["next_online"])
        if (gap > bound).all():
            return d, seed
    raise AssertionError(f"B{B} A{A} N{N} n{n_step}: no seed under {MAX_SEEDS} without a near-tie of the selection")


# network shapes of the float64 network test: (S, A, H, E, N, B)
NET_SHAPES = [(4, 3, 64, 8, 4, 3), (8, 5, 36, 5, 7, 6), (4, 2, 128, 64, 64, 4)]
