"""Restatement of Munchausen DQN's loss (core/agent/m_dqn.py:29-59, agent/utils.py:29-39) with torch autograd on the CPU: the ground
truth of the M-DQN tests.  float64 is the truth; the same function in float32 is the torch-CPU comparator of fp64_truth's criterion.
tests/test_mdqn_cpu.py pins it to the reference's own learn() through the three fixtures (tools/gen_golden_mdqn.py), so the GPU tests
may lean on it at shapes that have no fixture.  No reference code is read.

Per row, x = q_target, x' = q_next_target, a = action, with the row maximum subtracted before every exp:
  lp = x[a] - (max x + tau log sum_k exp((x_k - max x) / tau))                    scaled log-policy of target(s) at the taken action
  pi = exp(log_softmax((x' - max x') / tau)),  lp'_k = x'_k - (max x' + tau log sum exp((x' - max x') / tau))
  y  = reward + alpha * clip(lp, l_0, 0) + (1 - done) * gamma * sum_k pi_k (x'_k - lp'_k)
  loss = mean_b smooth_l1(q[b, a] - y, beta 1);  max_Q = max_b q[b, a]"""
import numpy as np
import torch


def mdqn_truth(q, q_target, q_next_target, action, reward, done, gamma, alpha, tau, l_0, dtype=torch.float64):
    """Inputs as arrays ([B, A] x 3, [B] x 3); float32 inputs are taken at their exact values.  Actions are clamped into [0, A).
    -> dict(loss, max_Q, mun_mean, grad [B, A], target [B], log_policy [B], clipped [B] bool, linear [B] bool), numpy, in `dtype`."""
    c = lambda v: torch.as_tensor(np.asarray(v)).to(dtype)
    qv = c(q).clone().requires_grad_(True)
    B, A = qv.shape
    xt, xn = c(q_target), c(q_next_target)
    act = torch.as_tensor(np.asarray(action, dtype=np.float64).reshape(B)).long().clamp(0, A - 1)
    r, d = c(reward).reshape(B, 1), c(done).reshape(B, 1)
    one_hot = torch.eye(A, dtype=dtype)[act]
    qa = (qv * one_hot).sum(1, keepdim=True)
    with torch.no_grad():
        def scaled_log_softmax(x):
            mx = x.max(-1, keepdim=True)[0]
            return x - (mx + tau * torch.log(torch.exp((x - mx) / tau).sum(-1, keepdim=True)))

        lp = (scaled_log_softmax(xt) * one_hot).sum(-1, keepdim=True)
        mun = alpha * torch.clip(lp, min=l_0, max=0)
        nlp = scaled_log_softmax(xn)
        pi = torch.exp(torch.log_softmax((xn - xn.max(-1, keepdim=True)[0]) / tau, -1))
        soft = (pi * (xn - nlp)).sum(-1, keepdim=True)
        y = r + mun + (1 - d) * gamma * soft
    loss = torch.nn.functional.smooth_l1_loss(qa, y)
    loss.backward()
    n = lambda t: t.detach().numpy()
    return dict(loss=float(loss.detach()), max_Q=float(qa.detach().max()), mun_mean=float(mun.mean()), grad=n(qv.grad), target=n(y).reshape(B), log_policy=n(lp).reshape(B),
                clipped=n((lp < l_0) | (lp > 0)).reshape(B), linear=n((qa - y).abs() >= 1).reshape(B))


# ---------------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_mdqn_gpu.py.  256, 257 and 600 are the one-, two- and three-block boundaries of the finish launch.
HYPER = dict(gamma=0.99, alpha=0.9, tau=0.03, l_0=-1.0)
SWEEP = [(B, A, "plain") for B in (1, 7, 32, 255, 256, 257, 600) for A in (1, 2, 5, 18)] + [(32, 6, "wide"), (32, 6, "flat"), (32, 6, "tau1")]
# at these `plain` cases at least one row lies on each side of the log-policy clip and of the Huber knee
BOTH_SIDES = [(32, 2), (33, 6), (255, 3)]


def sweep_case(B, A, variant, seed=0):
    """Seeded float32 inputs: q values ~ N(0, 1), rewards from {-1, 0, 0.5, 1}, about 10 % done.  `wide`: q x 20 (the policy is one-hot,
    the log-policy clips almost everywhere), `flat`: q x 0.01 (|tau log pi| << |l_0|: no row clips), `tau1`: tau = 1.
    -> (dict of arrays q, q_target, q_next_target [B, A]; action, reward, done [B]), hyper dict."""
    rs = np.random.RandomState(100 * B + A + 1000003 * seed)
    q, qt, qn = (rs.randn(B, A).astype(np.float32) for _ in range(3))
    action = rs.randint(0, A, size=B).astype(np.float32)
    reward = rs.choice(np.array([-1.0, 0.0, 0.5, 1.0], dtype=np.float32), size=B)
    done = (rs.rand(B) < 0.1).astype(np.float32)
    hyper = dict(HYPER)
    scale = {"plain": 1.0, "wide": 20.0, "flat": 0.01, "tau1": 1.0}[variant]
    q, qt, qn = (np.float32(scale) * v for v in (q, qt, qn))
    if variant == "tau1":
        hyper["tau"] = 1.0
    return dict(q=q, q_target=qt, q_next_target=qn, action=action, reward=reward, done=done), hyper
