"""Float64 restatement of continuous soft actor-critic learning (core/agent/sac.py:161-269 on the policy of core/network/policy.py:38-55 and the
critic of core/network/q_network.py:23-39) with torch autograd on the CPU: the comparator of tests/test_sac_cpu.py and tests/test_sac_gpu.py
(test infrastructure, not the product).  Every function takes `dtype`: torch.float64 is the truth, torch.float32 the torch-CPU-fp32 comparator
that fp64_truth.vs_exact's criterion needs.

  Actor / Critic        forward-capable mirrors under the reference's keys; Actor(x) -> (mu, std), Actor.raw(x) -> (mu_raw, ls_raw)
  sample                (mu_raw, ls_raw, eps) -> a = tanh(mu + std eps), logp [B]; differentiable in mu_raw / ls_raw
  sample_backward       d(mu_raw), d(ls_raw) of sum(da * a) + (alpha / B) sum(logp) by autograd
  critic_loss           y, both losses, max_Q and d(loss_i)/d(q_i) from q, q_next [2, B], logp_next and alpha
  actor_seed            actor_loss, alpha_loss, mean_Q, entropy and d(actor_loss)/d(q_i) [2, B] (torch.min's backward: half each on a tie)
  alpha_adam_step       one torch.optim.Adam step of log_alpha from a given optimizer state, in float64
  critic_update         one whole critic update given state dicts, a batch, eps and alpha
  actor_update          one whole actor update (through BOTH critics' action inputs and through logp) and the alpha loss
  adam_step             one Adam step from a given optimizer state: the critics as the actor update sees them
and the case builders of the kernel and network tests, and the reader of the fixtures of tools/gen_golden_sac.py."""
from collections import OrderedDict

import numpy as np
import torch


class _Head(torch.nn.Module):
    def __init__(self, S, H):
        super().__init__()
        self.l = torch.nn.Linear(S, H)


class Actor(torch.nn.Module):
    def __init__(self, S, A, H):
        super().__init__()
        self.head = _Head(S, H)
        self.l = torch.nn.Linear(H, H)
        self.mu = torch.nn.Linear(H, A)
        self.log_std = torch.nn.Linear(H, A)

    def raw(self, x):
        h = torch.relu(self.l(torch.relu(self.head.l(x))))
        return self.mu(h), self.log_std(h)

    def forward(self, x):
        mu_raw, ls_raw = self.raw(x)
        return torch.clamp(mu_raw, -5.0, 5.0), torch.tanh(ls_raw).exp()


class Critic(torch.nn.Module):
    def __init__(self, S, A, H):
        super().__init__()
        self.head = _Head(S, H)
        self.e = torch.nn.Linear(A, H)
        self.l = torch.nn.Linear(2 * H, H)
        self.q = torch.nn.Linear(H, 1)

    def forward(self, x, a):
        cat = torch.cat([torch.relu(self.head.l(x)), torch.relu(self.e(a))], dim=-1)
        return self.q(torch.relu(self.l(cat)))


ACTOR_KEYS = ("head.l.weight", "head.l.bias", "l.weight", "l.bias", "mu.weight", "mu.bias", "log_std.weight", "log_std.bias")
CRITIC_KEYS = ("head.l.weight", "head.l.bias", "e.weight", "e.bias", "l.weight", "l.bias", "q.weight", "q.bias")


def shapes_of(net, S, A, H):
    if "actor" in net:
        return OrderedDict(zip(ACTOR_KEYS, ((H, S), (H,), (H, H), (H,), (A, H), (A,), (A, H), (A,))))
    return OrderedDict(zip(CRITIC_KEYS, ((H, S), (H,), (H, A), (H,), (H, 2 * H), (H,), (1, H), (1,))))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(dtype)


def build(cls, sd, dtype):
    """A mirror module of `cls` holding the state dict `sd` (arrays or tensors, the reference's keys) in `dtype`."""
    H, S = (int(v) for v in np.shape(sd["head.l.weight"]))
    A = int(np.shape(sd["mu.weight"])[0]) if cls is Actor else int(np.shape(sd["e.weight"])[1])
    m = cls(S, A, H).to(dtype)
    m.load_state_dict(OrderedDict((k, _t(v, dtype)) for k, v in sd.items()))
    return m


# ---------------------------------------------------------------------------------------------- the elementwise steps
def sample(mu_raw, ls_raw, eps, dtype=torch.float64):
    """sac.py:161-169 behind policy.py:38-55.  mu_raw / ls_raw may be tensors that require grad (kept as they are), eps is data.
    -> (a [B, A], logp [B])."""
    mu_raw = mu_raw if torch.is_tensor(mu_raw) and mu_raw.requires_grad else _t(mu_raw, dtype)
    ls_raw = ls_raw if torch.is_tensor(ls_raw) and ls_raw.requires_grad else _t(ls_raw, dtype)
    mu, std = torch.clamp(mu_raw, -5.0, 5.0), torch.tanh(ls_raw).exp()
    m = torch.distributions.Normal(mu, std)
    z = mu + _t(eps, dtype) * std  # Normal.rsample with the given standard normals
    a = torch.tanh(z)
    logp = m.log_prob(z) - torch.log(1 - a.pow(2) + 1e-7)
    return a, logp.sum(1)


def sample_backward(da, mu_raw, ls_raw, eps, alpha, dtype=torch.float64):
    """d / d(mu_raw), d / d(ls_raw) of sum(da * a) + (alpha / B) * sum_b logp_b: what reaches the actor's two heads in the actor step when the
    critics hand back `da` and the loss carries alpha * logp / B (sac.py:241-244).  -> (d_mu_raw, d_ls_raw, a, logp), detached."""
    mu_raw, ls_raw = _t(mu_raw, dtype).clone().requires_grad_(True), _t(ls_raw, dtype).clone().requires_grad_(True)
    a, logp = sample(mu_raw, ls_raw, eps, dtype)
    B = a.shape[0]
    coef = torch.tensor(alpha, dtype=dtype) / B
    ((_t(da, dtype) * a).sum() + coef * logp.sum()).backward()
    return mu_raw.grad.detach(), ls_raw.grad.detach(), a.detach(), logp.detach()


def critic_loss(q, q_next, logp_next, reward, done, gamma, alpha, dtype=torch.float64):
    """q, q_next [2, B], logp_next [B] -> dict(y [B], loss [2], max_Q, grad [2, B])   (sac.py:186-216)."""
    q = _t(q, dtype).clone().requires_grad_(True)
    qn, lp, r, d = _t(q_next, dtype), _t(logp_next, dtype).reshape(-1), _t(reward, dtype).reshape(-1), _t(done, dtype).reshape(-1)
    y = r + (1 - d) * gamma * (torch.min(qn[0], qn[1]) + torch.tensor(alpha, dtype=dtype) * (-lp))
    losses = [torch.nn.functional.mse_loss(q[i], y) for i in range(2)]
    sum(losses).backward()
    return dict(y=y.detach(), loss=torch.stack(losses).detach(), max_Q=y.max().detach(), grad=q.grad.detach())


def actor_seed(q, logp, alpha, log_alpha, target_entropy, dtype=torch.float64):
    """q [2, B], logp [B] -> dict(actor_loss, alpha_loss, mean_Q, entropy, grad [2, B], coef = d(actor_loss)/d(logp_b), alpha_grad)
    (sac.py:241-248).  alpha_grad = d(alpha_loss)/d(log_alpha) = mean(-logp - target_entropy)."""
    q = _t(q, dtype).clone().requires_grad_(True)
    lp = _t(logp, dtype).reshape(-1).clone().requires_grad_(True)
    entropy = -lp
    min_q = torch.min(q[0], q[1])
    loss = -((torch.tensor(alpha, dtype=dtype) * entropy) + min_q).mean()
    loss.backward()
    g = (entropy - target_entropy).detach().mean()
    return dict(actor_loss=loss.detach(), alpha_loss=(torch.tensor(log_alpha, dtype=dtype) * g), mean_Q=min_q.mean().detach(), entropy=entropy.mean().detach(),
                grad=q.grad.detach(), coef=lp.grad.detach(), alpha_grad=g)


def alpha_adam_step(log_alpha, grad, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """ONE torch.optim.Adam step of the single parameter log_alpha in float64, started from the given optimizer state (`step` steps taken so
    far, moments m and v).  -> (log_alpha, m, v) after the step, as Python floats."""
    p = torch.nn.Parameter(torch.tensor([float(log_alpha)], dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    if step > 0:
        opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor([float(m)], dtype=torch.float64),
                        "exp_avg_sq": torch.tensor([float(v)], dtype=torch.float64)}
    p.grad = torch.tensor([float(grad)], dtype=torch.float64)
    opt.step()
    st = opt.state[p]
    return float(p.detach()), float(st["exp_avg"]), float(st["exp_avg_sq"])


# ---------------------------------------------------------------------------------------------- whole updates
def critic_update(sd_actor, sd_critics, sd_target_critics, state, action, reward, next_state, done, eps, gamma, alpha, dtype=torch.float64):
    """sac.py:183-225: the next action and its logp from the ONLINE actor on next_state.
    -> dict(next_action, logp_next, y, q [2][B, 1], loss [2], max_Q, grads [2]{name: tensor})."""
    actor = build(Actor, sd_actor, dtype)
    cs = [build(Critic, sd, dtype) for sd in sd_critics]
    tcs = [build(Critic, sd, dtype) for sd in sd_target_critics]
    s, a, r, s2, d = _t(state, dtype), _t(action, dtype), _t(reward, dtype).reshape(-1, 1), _t(next_state, dtype), _t(done, dtype).reshape(-1, 1)
    with torch.no_grad():
        a2, lp2 = sample(*actor.raw(s2), eps, dtype)
        nq = torch.min(tcs[0](s2, a2), tcs[1](s2, a2))
        y = r + (1 - d) * gamma * (nq + torch.tensor(alpha, dtype=dtype) * (-lp2.reshape(-1, 1)))
    qs, losses, grads = [], [], []
    for c in cs:
        q = c(s, a)
        loss = torch.nn.functional.mse_loss(q, y)
        loss.backward()
        qs.append(q.detach())
        losses.append(loss.detach())
        grads.append(OrderedDict((k, p.grad.detach().clone()) for k, p in c.named_parameters()))
    return dict(next_action=a2, logp_next=lp2, y=y, q=qs, loss=losses, max_Q=y.max(), grads=grads)


def actor_update(sd_actor, sd_critics, state, eps, alpha, log_alpha, target_entropy, dtype=torch.float64, actor=None, critics=None):
    """sac.py:229-248 with the critics AFTER their step.  -> dict(action, logp, min_q, actor_loss, alpha_loss, mean_Q, entropy, alpha_grad,
    grads {name: tensor}: the ACTOR's parameter gradients).  actor / critics: modules to use instead of building them from state dicts (the
    actor's p.grad is left on them)."""
    actor = build(Actor, sd_actor, dtype) if actor is None else actor
    cs = [build(Critic, sd, dtype) for sd in sd_critics] if critics is None else critics
    for p in actor.parameters():
        p.grad = None
    s = _t(state, dtype)
    a, lp = sample(*actor.raw(s), eps, dtype)
    lp = lp.reshape(-1, 1)
    entropy = -lp
    min_q = torch.min(cs[0](s, a), cs[1](s, a))
    loss = -((torch.tensor(alpha, dtype=dtype) * entropy) + min_q).mean()
    loss.backward()
    g = (entropy - target_entropy).detach().mean()
    return dict(action=a.detach(), logp=lp.detach().reshape(-1), min_q=min_q.detach(), actor_loss=loss.detach(), alpha_loss=torch.tensor(log_alpha, dtype=dtype) * g,
                mean_Q=min_q.mean().detach(), entropy=entropy.mean().detach(), alpha_grad=g,
                grads=OrderedDict((k, p.grad.detach().clone()) for k, p in actor.named_parameters()))


def adam_step(sd, grads, lr, m=None, v=None, step=0, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """One torch.optim.Adam step on the parameters `sd` with the gradients `grads` ({name: array}) in `dtype`, from a fresh optimizer (step 0)
    or from the moments m, v after `step` steps: what critic_optimizer{1,2}.step() leave behind (sac.py:219-225) in front of the actor
    update.  -> the stepped state dict."""
    params = OrderedDict((k, torch.nn.Parameter(_t(val, dtype).clone())) for k, val in sd.items())
    opt = torch.optim.Adam(list(params.values()), lr=lr, betas=betas, eps=eps)
    for k, p in params.items():
        p.grad = _t(grads[k], dtype).clone().reshape(p.shape)
        if step > 0:
            opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": _t(m[k], dtype).clone().reshape(p.shape), "exp_avg_sq": _t(v[k], dtype).clone().reshape(p.shape)}
    opt.step()
    return OrderedDict((k, p.detach().clone()) for k, p in params.items())


def polyak(p, t, tau):
    """The reference's expression (sac.py:273), evaluated by torch on tensors of the dtype given."""
    return tau * p + (1 - tau) * t


# ---------------------------------------------------------------------------------------------- case builders
SAMPLE_SHAPES = ((1, 1), (7, 3), (128, 6), (257, 2), (1025, 17))
SPREADS = (0.5, 1.5)
LOSS_B = (1, 7, 256, 257, 1025)
LOSS_VARIANTS = ("plain", "all_done", "equal_q")
ALPHA = 0.3                      # the temperature of the backward tests
WELL = 1e-3                      # 1 - a^2 >= WELL in the truth: the element's gradient is well conditioned
NET_SHAPES = [(3, 1, 32, 7), (11, 3, 64, 32), (17, 6, 256, 128), (4, 1, 512, 4)]


def sample_case(B, A, s):
    """mu_raw = 2 s randn, ls_raw = s randn, eps = randn from torch.Generator().manual_seed(0), rounded to float32, with two planted elements:
    element 0 (mu_raw 7, ls_raw 0, eps -3) is clamped and well conditioned: z = 2; element 1, where it exists, (mu_raw -5 exactly, eps 3.5)
    sits ON the clamp's bound, where the gradient passes.  -> float32 arrays mu_raw, ls_raw, eps [B, A]."""
    g = torch.Generator().manual_seed(0)
    mu = (2 * s * torch.randn(B, A, generator=g, dtype=torch.float64)).float().numpy()
    ls = (s * torch.randn(B, A, generator=g, dtype=torch.float64)).float().numpy()
    eps = torch.randn(B, A, generator=g, dtype=torch.float64).float().numpy()
    fm, fl, fe = mu.reshape(-1), ls.reshape(-1), eps.reshape(-1)
    fm[0], fl[0], fe[0] = 7.0, 0.0, -3.0
    if fm.size > 1:
        fm[1], fe[1] = -5.0, 3.5
    return mu, ls, eps


def sample_da(B, A):
    return torch.randn(B, A, generator=torch.Generator().manual_seed(1 + B + A), dtype=torch.float64).float().numpy()


def logp_bound(eps, a64, K):
    """K * 2^-24 * sum_j [4 + eps_j^2 + 2 / (1 - a_j^2 + 1e-7)] per row: the float32 rounding of each term of logp, plus a rounding error of
    a amplified through log(1 - a^2 + 1e-7)."""
    e, a = np.asarray(eps, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    return K * 2.0 ** -24 * (4 + e * e + 2 / (1 - a * a + 1e-7)).sum(1)


def loss_case(B, variant, seed=0):
    """q, q_next [2, B], logp, logp_next [B], reward, done [B] as float32 arrays.  equal_q: q1 == q2 (and q1' == q2') on every row."""
    rng = np.random.RandomState(91 * B + seed)
    q = rng.randn(2, B).astype(np.float32) * 2
    qn = rng.randn(2, B).astype(np.float32) * 2
    if variant == "equal_q":
        q[1], qn[1] = q[0], qn[0]
    lp = (rng.randn(B) * 2 - 1).astype(np.float32)
    lpn = (rng.randn(B) * 2 - 1).astype(np.float32)
    r = rng.choice([-1.0, 0.0, 1.0, 0.5], size=B).astype(np.float32)
    d = np.ones(B, np.float32) if variant == "all_done" else (rng.rand(B) < 0.2).astype(np.float32)
    return q, qn, lp, lpn, r, d


def mirrors(cls, S, A, H, seed):
    """A float64 mirror with float32-representable weights (torch's default Linear init under `seed`, biases perturbed) and its float32 copy."""
    import fp64_truth as T

    torch.manual_seed(seed)
    m = cls(S, A, H).double()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    T.round_to_fp32_(m)
    return m, T.as32(m)


def net_inputs(S, A, B, n):
    """The inputs of the network test, from one generator: n critic steps (x_all [2B, S], action, reward, done, eps) and n actor steps
    (x [B, S], eps).  eps is drawn narrow (0.6 randn, clamped to +-1.2) so that max |z| stays below 4: saturation is the elementwise tests'
    ground."""
    g = torch.Generator().manual_seed(1)
    eps = lambda: (0.6 * torch.randn(B, A, generator=g)).clamp(-1.2, 1.2)
    x0, act0 = torch.randn(B, S, generator=g), torch.tanh(torch.randn(B, A, generator=g))
    critic = [dict(x_all=torch.randn(2 * B, S, generator=g), action=torch.tanh(torch.randn(B, A, generator=g)), reward=torch.randn(B, generator=g),
                   done=(torch.rand(B, generator=g) < 0.2).float(), eps=eps()) for _ in range(n)]
    actor = [dict(x=torch.randn(B, S, generator=g), eps=eps()) for _ in range(n)]
    return x0, act0, critic, actor


# ---------------------------------------------------------------------------------------------- fixtures (tools/gen_golden_sac.py)
# the configuration of the learning-curve comparison: what tools/gen_golden_sac.py ran the reference with (the fixture stores it and both test files
# compare) and what the GPU test builds the HIP agent from
CURVE_CONFIG = dict(S=11, A=3, steps=12000, chunk=1000, run_step=15000, hidden=256, batch=128, buffer=50000, start=1000, tau=5e-3, gamma=0.99, lr_decay=True,
                    sac=dict(use_dynamic_alpha=True, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=3e-4),
                    note="12000 steps, not TD3's 8000: over 8000 the reference's own three seeds rise by 0.27, short of the 0.3 that 'learns' asks for")
FIXTURES = ("sac", "sac_odd", "sac_pendulum")
FIXTURE_NETS = ("actor", "critic1", "target_critic1", "critic2", "target_critic2")  # the reference's construction order (sac.py:75-95)


class Fixture:
    """One fixture file: the starting weights of every network in full (stored, or regenerated from the recipe and checked against the
    stored sample), the thinning rule of everything else, and the records."""

    def __init__(self, z):
        from oracle import synth

        self.z = z
        self.S, self.A, self.H, self.B = (int(z[f"hyper/{k}"]) for k in ("S", "A", "H", "B"))
        self.limit = int(z["hyper/thin_limit"])
        self.dynamic = bool(int(z["hyper/use_dynamic_alpha"]))
        self.nets = FIXTURE_NETS
        self.records = sorted({k.split("/")[0] for k in z.files if k.startswith("r") and k.split("/")[0][1:].isdigit()})
        self.sd0 = {}
        for i, net in enumerate(self.nets):
            shapes = shapes_of(net, self.S, self.A, self.H)
            if int(z["hyper/recipe"]):
                sd = synth.recipe_state_dict(shapes, int(z["hyper/recipe_seed"]) + i)
                if net == "actor":  # the generator scales the two head matrices down
                    for k in ("mu.weight", "log_std.weight"):
                        sd[k] = sd[k] * np.float32(float(z["hyper/head_scale"]))
                for k, v in sd.items():
                    assert np.array_equal(self.thin(v), z[f"sd0/{net}/{k}"]), (net, k)
            else:
                sd = OrderedDict((k, z[f"sd0/{net}/{k}"]) for k in shapes)
                assert all(tuple(sd[k].shape) == tuple(s) for k, s in shapes.items())
            self.sd0[net] = OrderedDict((k, np.asarray(sd[k], dtype=np.float32)) for k in shapes)

    def thin(self, a):
        from oracle import synth

        a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
        return synth.thin(a, self.limit) if self.limit else a

    def batch(self, r):
        return {k: self.z[f"{r}/learn/{k}"] for k in ("state", "action", "reward", "next_state", "done")}

    def eps(self, r):
        """[2, B, A]: the draw of the critic target, then the actor step's."""
        return np.stack([self.z[f"{r}/learn/eps_target"], self.z[f"{r}/learn/eps_actor"]])

    def full(self, r, net):
        """The weights of `net` after record r, in full -- stored only by a fixture that is not thinned (r1 of sac.npz starts there)."""
        assert not self.limit
        if int(self.z[f"{r}/unchanged/{net}"]):
            return self.sd0[net]
        return OrderedDict((k, self.z[f"{r}/sd1/{net}/{k}"]) for k in self.sd0[net])

    def start(self, r):
        """{net: state dict} at the start of record r: the fixture's sd0, or where the record before ended."""
        i = self.records.index(r)
        return dict(self.sd0) if i == 0 else {net: self.full(self.records[i - 1], net) for net in self.nets}

    def moments(self, r, net):
        """(exp_avg, exp_avg_sq) {name: array} of `net` ("actor", "critic1", "critic2") after record r, as stored (thinned where the fixture is)."""
        return tuple(OrderedDict((k, self.z[f"{r}/opt/{net}/{kind}/{k}"]) for k in self.sd0[net]) for kind in ("exp_avg", "exp_avg_sq"))

    def alpha(self, r, when):
        """The temperature before (when 0) / after (1) record r: dict(log_alpha, alpha, step, exp_avg, exp_avg_sq)."""
        return {k: self.z[f"{r}/alpha{when}/{k}"].item() for k in ("log_alpha", "alpha", "step", "exp_avg", "exp_avg_sq")}

    def buffer(self):
        """The stored transitions as the list of dicts an agent's process / memory.store takes."""
        z = self.z
        n = len(z["buf_state"])
        return [{k: z[f"buf_{k}"][i : i + 1] for k in ("state", "action", "reward", "next_state", "done")} for i in range(n)]

