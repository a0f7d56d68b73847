"""Restatement of IQN (core/network/iqn.py:9-47, core/agent/iqn.py:78-146) with torch autograd on the CPU: the ground truth of the IQN
tests.  float64 is the truth; the same functions in float32 are the torch-CPU comparator of fp64_truth's criterion.
tests/test_iqn_cpu.py pins them to the reference's own learn() through the three fixtures (tools/gen_golden_iqn.py), so the GPU tests
may lean on them at shapes that have no fixture.  No reference code is read.

Network, for R rows, N samples per row, E cosine features, width H, A actions:
  feat = relu(head.l(x)),  psi = relu(state_embed(feat))                                     [R, H]
  arg  = float32(tau * i_pi),  i_pi = float32(arange(E)) * float32(pi)                       [R, N, E]   -- the ARGUMENT is a float32 product
  phi  = relu(sample_embed(cos(arg))),  embed = psi[:, None, :] * phi                        [R, N, H]      in every precision; the cosine and
  logits = q(relu(l2(relu(l1(embed)))))                                                      [R, N, A]      everything after it is `dtype`
Loss, with P[b, i] = logit[b, i, action[b]], a*[b] = first argmax_a mean_n next_online[b, n, a],
T[b, j] = reward[b] + (1 - done[b]) * gamma * target[b, j, a*[b]], e[b, j, i] = T[b, j] - P[b, i]:
  loss = 1 / (B N) * sum_{b, j, i} (1 - tau[b, i] if e < 0 else tau[b, i]) * smooth_l1(e),  tau = the draw of the forward that gave `logit`."""
import numpy as np
import torch

KEYS = ("head.l.weight", "head.l.bias", "state_embed.weight", "state_embed.bias", "sample_embed.weight", "sample_embed.bias", "l1.weight", "l1.bias",
        "l2.weight", "l2.bias", "q.weight", "q.bias")


def i_pi(E):
    """arange(0, E) * np.pi as the reference's float32 tensor holds it (iqn.py:14)."""
    return np.arange(E, dtype=np.float32) * np.float32(np.pi)


def cos_argument(tau, E):
    """float32 [..., E]: the product tau * i_pi rounded to float32, whatever precision takes the cosine afterwards."""
    t = np.asarray(tau, dtype=np.float32)
    return (t[..., None] * i_pi(E)).astype(np.float32)


def cos_features(tau, E, dtype=torch.float64):
    return torch.cos(torch.from_numpy(cos_argument(tau, E)).to(dtype))


def iqn_forward(sd, x, tau, dtype=torch.float64):
    """sd: {state_dict key: tensor} (used as they are when they already have `dtype`, so that leaves with requires_grad stay leaves);
    x [R, S]; tau float32 [R, N].  -> logits [R, N, A] in `dtype`, with the graph attached."""
    w = {k: (v if torch.is_tensor(v) and v.dtype == dtype else torch.as_tensor(np.asarray(v)).to(dtype)) for k, v in sd.items()}
    F = torch.nn.functional
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    E = w["sample_embed.weight"].shape[1]
    feat = F.relu(F.linear(x, w["head.l.weight"], w["head.l.bias"]))
    psi = F.relu(F.linear(feat, w["state_embed.weight"], w["state_embed.bias"]))
    phi = F.relu(F.linear(cos_features(tau, E, dtype), w["sample_embed.weight"], w["sample_embed.bias"]))
    h = psi.unsqueeze(1) * phi
    h = F.relu(F.linear(h, w["l1.weight"], w["l1.bias"]))
    h = F.relu(F.linear(h, w["l2.weight"], w["l2.bias"]))
    return F.linear(h, w["q.weight"], w["q.bias"])


def iqn_loss(logit, next_online, target, action, reward, done, tau, gamma, dtype=torch.float64, a_star=None):
    """Inputs as arrays or tensors ([B, N, A] x 3, [B] x 3, tau float32 [B, N]); float32 inputs are taken at their exact values.  When
    `logit` is a tensor with a graph, the loss is attached to it (backward through a network); otherwise d loss / d logit is returned.
    a_star: use these next actions instead of the argmax (to score a kernel's loss on rows where the selection is a near-tie).
    -> dict(loss_t (tensor), loss, grad [B, N, A] | None, a_star [B], max_Q, max_logit, min_logit, gap [B], gap_bound [B], abs_e_min, abs_e_max)."""
    c = lambda v: v.to(dtype) if torch.is_tensor(v) else torch.as_tensor(np.asarray(v)).to(dtype)
    attached = torch.is_tensor(logit) and logit.requires_grad
    z = logit if attached else c(logit).clone().requires_grad_(True)
    zn, zt = c(next_online).detach(), c(target).detach()
    B, N, A = z.shape
    act = torch.as_tensor(np.asarray(action, dtype=np.float64).reshape(B)).long().clamp(0, A - 1)
    r, d = c(reward).reshape(B, 1), c(done).reshape(B, 1)
    tau32 = torch.as_tensor(np.asarray(tau, dtype=np.float32).reshape(B, N))
    inv_tau = (1 - tau32).to(dtype)  # the reference forms 1 - tau in float32 (iqn.py:120)
    tau_t = tau32.to(dtype)
    rows = torch.arange(B)
    qn = zn.mean(1)
    best = qn.argmax(-1)  # first maximum
    sel = best if a_star is None else torch.as_tensor(np.asarray(a_star)).long().reshape(B)
    P = z[rows, :, act]  # [B, N] (i)
    T = r + (1 - d) * gamma * zt[rows, :, sel]  # [B, N] (j)
    e = T[:, :, None] - P[:, None, :]  # [B, j, i]
    hub = torch.nn.functional.smooth_l1_loss(*torch.broadcast_tensors(P[:, None, :], T[:, :, None]), reduction="none")
    wgt = torch.where(e < 0, inv_tau[:, None, :], tau_t[:, None, :])
    loss = (wgt * hub).sum(2).mean()
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
    ae = e.detach().abs()
    return dict(loss_t=loss, loss=float(loss.detach()), grad=grad, a_star=best.numpy(), max_Q=float(zd.mean(1).max()), max_logit=float(zd.max()), min_logit=float(zd.min()),
                gap=gap, gap_bound=gap_bound, abs_e_min=float(ae.min()), abs_e_max=float(ae.max()))


def hadamard_backward(psi_pre, phi_pre, grad_embed, dtype=torch.float64):
    """embed = relu(psi_pre)[:, None, :] * relu(phi_pre) -> (d psi_pre [B, H], d phi_pre [B, N, H]) for d embed = grad_embed, by autograd."""
    p = torch.as_tensor(np.asarray(psi_pre)).to(dtype).requires_grad_(True)
    f = torch.as_tensor(np.asarray(phi_pre)).to(dtype).requires_grad_(True)
    (torch.relu(p).unsqueeze(1) * torch.relu(f)).backward(torch.as_tensor(np.asarray(grad_embed)).to(dtype))
    return p.grad, f.grad


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_iqn_gpu.py (inputs only; the CPU suite checks its properties before a GPU sees them).
SWEEP_SHAPES = [(1, 1, 1), (7, 5, 33), (32, 2, 64), (255, 6, 51), (3, 4, 256)]  # (B, A, N)
VARIANTS = ("plain", "all_done", "large")
SWEEP = [(B, A, N, v) for (B, A, N) in SWEEP_SHAPES for v in VARIANTS]


def sweep_case(B, A, N, variant, seed=0):
    """Seeded float32 inputs: logits ~ N(0, 1), rewards from {-1, 0, 0.5, 1}, about 10 % done, tau ~ U(0, 1) per (row, sample).
    `all_done`: done = 1 on every row (T[b, :] = reward[b]); `large`: logits x 0.05 and reward 5, so that |e| > 1 for every pair.
    -> dict of arrays (logit, next_online, target [B, N, A]; action, reward, done [B]; tau [B, N])."""
    rs = np.random.RandomState(1000003 * seed + 7919 * B + 131 * A + N + 17)
    z, zn, zt = (rs.randn(B, N, A).astype(np.float32) for _ in range(3))
    action = rs.randint(0, A, size=B).astype(np.float32)
    reward = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32), size=B)
    done = (rs.rand(B) < 0.1).astype(np.float32)
    tau = rs.rand(B, N).astype(np.float32)
    if variant == "all_done":
        done[:] = 1.0
    if variant == "large":
        z, zn, zt = (np.float32(0.05) * v for v in (z, zn, zt))
        reward[:] = 5.0
    return dict(logit=z, next_online=zn, target=zt, action=action, reward=reward, done=done, tau=tau)


# network shapes of the float64 network test: (S, A, H, E, N, B); together: B * N not a multiple of the tile, E not a multiple of 4, the reference's width
NET_SHAPES = [(4, 3, 32, 16, 8, 32), (6, 5, 64, 10, 33, 7), (4, 2, 512, 64, 64, 4)]
