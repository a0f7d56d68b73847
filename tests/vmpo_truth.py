"""Float64 restatement of one V-MPO minibatch update (core/agent/vmpo.py:155-252 on the policy modules of core/network/policy_value.py:8-57)
with torch autograd on the CPU: the comparator of tests/test_vmpo_cpu.py and tests/test_vmpo_gpu.py (test infrastructure, not the product).
Every function takes `dtype`: torch.float64 is the truth, torch.float32 the torch-CPU-fp32 comparator that fp64_truth's criterion needs.

  loss                  the four losses, the top half, d(loss)/d(raw heads) and d(loss)/d(eta, alpha_mu, alpha_sigma) from a minibatch's raw heads,
                        the old raw heads of its rows, actions, advantages, old values and the three multipliers
  multiplier_step       one torch.optim.Adam step of one scalar from a given optimizer state in float64, then max(x, floor) (reset_lgr_muls)
  update                one whole minibatch update through a mirror module (tests/mirror): heads, losses, parameter gradients
  prepass               vmpo.py:122-153: old raw heads, values, GAE, per-row standardisation (the fixtures' check of the upstream quantities)
and the case builders of the kernel tests, and the reader of the fixtures of tools/gen_golden_vmpo.py.

What is taken as INPUT PREPARATION, done in float32 whatever `dtype` (it is float32 tensor arithmetic in the reference, and the kernels do the same
single operations): the action clamp to +-(1 - 1e-7), ret = adv + value_old, and the lower median with the strict `>` (exact in any dtype)."""
from collections import OrderedDict

import numpy as np
import torch

NAMES = ("eta", "alpha_mu", "alpha_sigma")
EPS_DEFAULT = (0.02, 0.1, 0.1)


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(dtype)


def top_half(adv):
    """(lower median, boolean mask adv > median) of a float32 minibatch of advantages, by torch itself (vmpo.py:174)."""
    a = torch.as_tensor(np.asarray(adv, dtype=np.float32)).reshape(-1)
    med = a.median()
    return float(med), (a > med).numpy()


def loss(cont, heads, old, action, adv, value_old, mult, eps=EPS_DEFAULT, dtype=torch.float64):
    """heads {"logits" | "mu_raw", "log_std_raw", "v"}: the minibatch's raw heads [b, A] / [b]; old: the same keys (no "v") for the OLD policy on the
    same rows; action [b, 1] | [b, A]; adv, value_old [b]; mult = (eta, alpha_mu, alpha_sigma).
    -> dict(actor, critic, eta_loss, alpha_loss: floats; med; top [b] bool; grads {head: array}; mult_grads [3] (alpha_sigma's None when
    discrete: it has no gradient, vmpo.py:236-242); mult_scale: the magnitude of those gradients' terms; kl: the per-row KL terms)."""
    adv32 = torch.as_tensor(np.asarray(adv, dtype=np.float32)).reshape(-1, 1)
    vold32 = torch.as_tensor(np.asarray(value_old, dtype=np.float32)).reshape(-1, 1)
    ret = (adv32 + vold32).to(dtype)  # vmpo.py:153, float32
    _adv = adv32.to(dtype)
    med = adv32.median()
    idx_tophalf = adv32 > med
    m3 = [torch.tensor(float(np.float32(x)), dtype=dtype, requires_grad=True) for x in mult]
    eta, alpha_mu, alpha_sigma = m3
    eps_eta, eps_alpha_mu, eps_alpha_sigma = (float(np.float32(e)) for e in eps)
    value = _t(heads["v"], dtype).reshape(-1, 1).requires_grad_(True)

    tophalf_adv = _adv[idx_tophalf]
    exp_adv_eta = torch.exp(tophalf_adv / eta)
    psi = exp_adv_eta / torch.sum(exp_adv_eta.detach())
    if cont:
        mu_raw, ls_raw = _t(heads["mu_raw"], dtype).requires_grad_(True), _t(heads["log_std_raw"], dtype).requires_grad_(True)
        leaves = {"mu_raw": mu_raw, "log_std_raw": ls_raw, "v": value}
        mu, std = torch.clamp(mu_raw, -5.0, 5.0), torch.tanh(ls_raw).exp()
        _mu_old, _std_old = torch.clamp(_t(old["mu_raw"], dtype), -5.0, 5.0), torch.tanh(_t(old["log_std_raw"], dtype)).exp()
        m = torch.distributions.Normal(mu, std)
        a_cl = torch.clamp(torch.as_tensor(np.asarray(action, dtype=np.float32)), -1 + 1e-7, 1 - 1e-7).to(dtype)
        log_prob = m.log_prob(torch.atanh(a_cl)).sum(-1, keepdim=True)
    else:
        logits = _t(heads["logits"], dtype).requires_grad_(True)
        leaves = {"logits": logits, "v": value}
        pi = torch.exp(torch.log_softmax(logits, dim=-1))
        _pi_old = torch.exp(torch.log_softmax(_t(old["logits"], dtype), dim=-1))
        _log_pi_old = torch.log(_pi_old)
        log_prob = torch.log(pi.gather(1, torch.as_tensor(np.asarray(action)).reshape(-1, 1).long()))
        log_pi = torch.log(pi)
    critic_loss = torch.nn.functional.mse_loss(value, ret).mean()
    eta_loss = eta * eps_eta + eta * torch.log(torch.mean(exp_adv_eta))
    tophalf_log_prob = log_prob[idx_tophalf.squeeze(1), :]
    actor_loss = -torch.sum(psi.detach().unsqueeze(1) * tophalf_log_prob)
    if cont:
        ss, ss_old = 1.0 / (std ** 2), 1.0 / (_std_old ** 2)
        d_mu = mu - _mu_old
        KLD_mu = 0.5 * torch.sum(d_mu * 1.0 / ss_old * d_mu, axis=1)
        mu_loss = torch.mean(alpha_mu * (eps_alpha_mu - KLD_mu.detach()) + alpha_mu.detach() * KLD_mu)
        KLD_sigma = 0.5 * (torch.sum(1.0 / ss * ss_old, axis=1) - ss.shape[-1] + torch.log(torch.prod(ss, axis=1) / torch.prod(ss_old, axis=1)))
        sigma_loss = torch.mean(alpha_sigma * (eps_alpha_sigma - KLD_sigma.detach()) + alpha_sigma.detach() * KLD_sigma)
        alpha_loss = mu_loss + sigma_loss
        kl = (KLD_mu.detach().numpy(), KLD_sigma.detach().numpy())
    else:
        KLD_pi = torch.sum(_pi_old * (_log_pi_old - log_pi), axis=1)
        alpha_loss = torch.mean(alpha_mu * (eps_alpha_mu - KLD_pi.detach()) + alpha_mu.detach() * KLD_pi)
        kl = (KLD_pi.detach().numpy(),)
    total = critic_loss + actor_loss + eta_loss + alpha_loss
    total.backward()
    # the multipliers' gradients are DIFFERENCES -- eps_eta + log mean exp(adv / eta) - sum psi adv / eta, and eps_alpha - mean KL --: an error is
    # measured against the sum of the magnitudes of their terms, which is what a float32 evaluation rounds
    with torch.no_grad():
        mult_scale = [eps_eta + float(torch.log(torch.mean(exp_adv_eta)).abs()) + float((psi * tophalf_adv).sum().abs() / eta) if tophalf_adv.numel() else float("nan")]
        mult_scale += [e + float(np.mean(k_)) for e, k_ in zip((eps_alpha_mu, eps_alpha_sigma), kl)]
    return dict(actor=float(actor_loss.detach()), critic=float(critic_loss.detach()), eta_loss=float(eta_loss.detach()), alpha_loss=float(alpha_loss.detach()),
                med=float(med), top=idx_tophalf.reshape(-1).numpy(), grads={k: x.grad.detach().numpy() for k, x in leaves.items()},
                mult_grads=[None if x.grad is None else float(x.grad) for x in m3], mult_scale=mult_scale, kl=kl)


def multiplier_step(x, grad, m, v, step, lr, floor, betas=(0.9, 0.999), eps=1e-8):
    """ONE torch.optim.Adam step of one scalar in float64 from the given optimizer state (`step` steps taken so far), then max(x, floor) as
    torch.max does it (a NaN stays).  -> (x, m, v) as Python floats."""
    p = torch.nn.Parameter(torch.tensor(float(x), dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps)
    if step > 0:
        opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor(float(m), dtype=torch.float64), "exp_avg_sq": torch.tensor(float(v), dtype=torch.float64)}
    p.grad = torch.tensor(float(grad), dtype=torch.float64)
    opt.step()
    st = opt.state[p]
    return float(torch.max(p.detach(), torch.tensor(float(floor), dtype=torch.float64))), float(st["exp_avg"]), float(st["exp_avg_sq"])


def update(module, cont, x, old, action, adv, value_old, mult, eps=EPS_DEFAULT):
    """One minibatch through a mirror module (tests/mirror/networks.py) in the module's own dtype: x [b, S] and the other arguments are the
    minibatch's gathered rows.  -> (loss(...)'s dict with the heads added, {parameter: d(loss)/d(parameter)} from the head gradients)."""
    dt = next(module.parameters()).dtype
    for p in module.parameters():
        p.grad = None
    raw = module.raw(_t(x, dt))
    names = ("mu_raw", "log_std_raw", "v") if cont else ("logits", "v")
    heads = {k: h.detach().numpy() for k, h in zip(names, raw)}
    out = loss(cont, heads, old, action, adv, value_old, mult, eps, dt)
    torch.autograd.backward(list(raw), [torch.as_tensor(out["grads"][k]).reshape(h.shape) for k, h in zip(names, raw)])
    out["heads"] = heads
    return out, OrderedDict((k, p.grad.detach().clone()) for k, p in module.named_parameters())


def prepass(module, cont, state, next_state, reward, done, n_step, gamma, lam, standardize=True):
    """vmpo.py:122-153 in the module's dtype -> dict(old raw heads, value, adv [M]); ret is left to loss()."""
    dt = next(module.parameters()).dtype
    with torch.no_grad():
        raw = module.raw(_t(state, dt))
        value = raw[-1]
        next_value = module.raw(_t(next_state, dt))[-1]
        reward, done = _t(reward, dt).reshape(-1, 1), _t(done, dt).reshape(-1, 1)
        delta = reward + (1 - done) * gamma * next_value - value
        adv = delta.clone()
        adv, done = adv.view(-1, n_step), done.view(-1, n_step)
        for t in reversed(range(n_step - 1)):
            adv[:, t] += (1 - done[:, t]) * gamma * lam * adv[:, t + 1]
        if standardize:
            adv = (adv - adv.mean(dim=1, keepdim=True)) / (adv.std(dim=1, keepdim=True) + 1e-7)
    names = ("mu_raw", "log_std_raw") if cont else ("logits",)
    out = {k: h.numpy() for k, h in zip(names, raw)}
    out.update(value=value.reshape(-1).numpy(), adv=adv.reshape(-1).numpy())
    return out


# ---------------------------------------------------------------------------------------------- case builders
LOSS_B = (2, 3, 8, 63, 64, 65, 255, 256, 257, 1024)  # the kernel has ONE path: a block of b rounded up to 64 threads; 63/64/65, 255/256/257 straddle wave and 4-wave counts
DISCRETE_A = (2, 6)
CONTINUOUS_A = (1, 3, 17)
VARIANTS = ("plain", "ties", "all_equal", "hot", "clamped", "floor")
MULT = (2.0, 0.5, 3.0)
FLOORS = (1e-8, 1e-8, 1e-8)
LR, BETAS, ADAM_EPS, STEP0 = 3e-3, (0.9, 0.999), 1e-8, 3  # the kernel tests' hand-made optimizer block: three steps already taken


def case(cont, b, A, variant, seed=0):
    """One kernel-test case: a rollout of M = 2 b + 3 rows, a non-trivial idx (b distinct rows of a permutation), the minibatch's new heads near
    the old ones.  -> dict of float32 / int64 arrays: idx [b], adv, value_old [M], action, old heads [M, .], heads of the minibatch [b, .],
    mult, floors, m, v (the multipliers' optimizer state before the step)."""
    rng = np.random.RandomState(1000 * b + 10 * A + seed + (7 if cont else 0))
    M = 2 * b + 3
    idx = rng.permutation(M)[:b].astype(np.int64)
    adv = rng.randn(M).astype(np.float32)
    mult, floors = list(MULT), list(FLOORS)
    m, v = [0.01, -0.02, 0.005], [1e-4, 4e-4, 1e-4]
    if variant == "ties" and b >= 3:
        # several rows bit-equal to the lower median, and duplicates above it
        order = idx[np.argsort(adv[idx], kind="stable")]
        k = (b - 1) // 2
        med = adv[order[k]]
        for j in range(max(0, k - 2), min(b, k + 2)):
            adv[order[j]] = med
        if k + 3 < b:
            adv[order[k + 3]] = adv[order[b - 1]]
            adv[order[k + 2]] = adv[order[b - 1]]
    elif variant == "all_equal":
        adv[:] = np.float32(0.37)
    elif variant == "hot":
        mult[0] = 0.02  # adv up to ~3: adv / eta up to 150
        adv[idx[0]] = np.float32(3.0)
    elif variant == "floor":
        # eta's gradient is positive here (eps_eta + log mean - sum psi adv / eta with adv / eta small): a step of ~lr down from just above the floor crosses it
        floors = [1.0, 0.2, 1.0]
        mult = [1.0 + 1e-4, 0.2 + 1e-4, 1.0 + 1e-4]
        m, v = [0.5, 0.5, 0.5], [0.25, 0.25, 0.25]
    value_old = rng.randn(M).astype(np.float32)
    out = dict(idx=idx, adv=adv, value_old=value_old, mult=np.asarray(mult, np.float32), floors=np.asarray(floors, np.float32), m=np.asarray(m, np.float32),
               v=np.asarray(v, np.float32), v_pred=(value_old[idx] + 0.3 * rng.randn(b)).astype(np.float32))
    if cont:
        out["action"] = np.tanh(rng.randn(M, A)).astype(np.float32)
        out["mu_raw_old"] = rng.randn(M, A).astype(np.float32)
        out["log_std_raw_old"] = (0.5 * rng.randn(M, A)).astype(np.float32)
        out["mu_raw"] = (out["mu_raw_old"][idx] + 0.2 * rng.randn(b, A)).astype(np.float32)
        out["log_std_raw"] = (out["log_std_raw_old"][idx] + 0.2 * rng.randn(b, A)).astype(np.float32)
        if variant == "clamped":
            out["mu_raw"][::2, 0] = np.float32(6.5)       # beyond the clamp: no gradient
            out["mu_raw"][1::2, 0] = np.float32(-5.0)     # ON the bound: the gradient passes
            out["mu_raw_old"][idx[::3], 0] = np.float32(-7.0)
            out["action"][idx[::2], A - 1] = np.float32(1.0)
            out["action"][idx[1::2], 0] = np.float32(-1.0)
    else:
        out["action"] = rng.randint(0, A, size=(M, 1)).astype(np.float32)
        out["logits_old"] = rng.randn(M, A).astype(np.float32)
        out["logits"] = (out["logits_old"][idx] + 0.3 * rng.randn(b, A)).astype(np.float32)
    return out


def case_truth(cont, c, dtype=torch.float64):
    idx = c["idx"]
    if cont:
        heads, old = {"mu_raw": c["mu_raw"], "log_std_raw": c["log_std_raw"], "v": c["v_pred"]}, {"mu_raw": c["mu_raw_old"][idx], "log_std_raw": c["log_std_raw_old"][idx]}
    else:
        heads, old = {"logits": c["logits"], "v": c["v_pred"]}, {"logits": c["logits_old"][idx]}
    return loss(cont, heads, old, c["action"][idx], c["adv"][idx], c["value_old"][idx], c["mult"], EPS_DEFAULT, dtype)


# ---------------------------------------------------------------------------------------------- fixtures (tools/gen_golden_vmpo.py)
FIXTURES = ("vmpo_discrete", "vmpo_continuous", "vmpo_cartpole")
MEDIAN_GAP = 1e-4  # the generator's condition: next larger advantage - median >= MEDIAN_GAP * max |adv| in every recorded minibatch
CURVE_CONFIG = dict(workers=8, n_step=128, iterations=40, seeds=(1, 2, 3), run_step=100000,
                    agent=dict(state_size=4, action_size=2, hidden_size=512, network="discrete_policy_value", optim_config={"name": "adam", "lr": 2.5e-4},
                               gamma=0.99, batch_size=64, n_step=128, n_epoch=1, _lambda=0.95, min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.02,
                               eps_alpha_mu=0.1, eps_alpha_sigma=0.1, eta=2.0, alpha_mu=0.1, alpha_sigma=5.0, lr_decay=True))  # config/vmpo/cartpole.py


def curve_gain(curve):
    """The summary of one learning curve: the mean of its last five iterations over its first iteration."""
    return float(np.mean(curve[-5:])) / float(curve[0])


class Fixture:
    """One fixture file of tools/gen_golden_vmpo.py: hyper-parameters, the rollout, starting weights (stored, or regenerated from the recipe and
    checked against the stored sample) and per learn `l<k>/` the pre-pass and per minibatch `l<k>/mb<i>/` what the reference computed."""

    def __init__(self, z):
        from oracle import synth

        self.z = z
        g = lambda k: z[f"hyper/{k}"].item()
        self.S, self.A, self.H, self.W, self.T, self.B = (int(g(k)) for k in ("S", "A", "H", "W", "T", "B"))
        self.cont = bool(int(g("continuous")))
        self.M = self.W * self.T
        self.limit = int(g("thin_limit"))
        self.recipe = bool(int(g("recipe")))
        self.learns = int(g("learns"))
        self.lr, self.gamma, self.lam, self.clip = float(g("lr")), float(g("gamma")), float(g("lambda")), float(g("clip_grad_norm"))
        self.mult0 = tuple(float(g(k)) for k in NAMES)
        self.floors = tuple(float(g("min_" + k)) for k in NAMES)
        self.eps = tuple(float(g("eps_" + k)) for k in NAMES)
        self.network = "continuous_policy_value" if self.cont else "discrete_policy_value"
        names = [k[len("sd0/"):] for k in z.files if k.startswith("sd0/")]
        if self.recipe:
            shapes = OrderedDict((k, tuple(int(s) for s in z[f"shape/{k}"])) for k in names)
            sd = synth.ppo_recipe(shapes, int(g("recipe_seed")))
            for k in names:
                assert np.array_equal(self.thin(sd[k]), z[f"sd0/{k}"]), k
            self.sd0 = OrderedDict((k, sd[k]) for k in names)
        else:
            self.sd0 = OrderedDict((k, z[f"sd0/{k}"]) for k in names)

    def thin(self, a):
        from oracle import synth

        a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
        return synth.thin(a, self.limit) if self.limit else a

    def n_minibatch(self):
        return (self.M + self.B - 1) // self.B

    def rollout(self, k):
        """The transitions of learn k as the list of dicts process() takes."""
        from oracle import synth

        z, p = self.z, f"l{k}/in_"
        if p + "state" in z.files:
            return [{key: z[p + key][i : i + 1] for key in ("state", "action", "reward", "next_state", "done")} for i in range(self.M)]
        # a recipe fixture: the rollout is regenerated from its seed and pinned by the stored checksums
        trs = synth.ppo_rollout(np.random.RandomState(int(z[f"l{k}/rollout_seed"])), self.M, self.S, self.A, self.cont, clamp_every=int(z["hyper/clamp_every"]))
        for key in ("state", "reward", "action"):
            got = synth.row_checksum(np.concatenate([t[key] for t in trs], 0).astype(np.float32))[:: max(1, self.M // 64)]
            assert np.array_equal(got, z[f"{p}{key}_check"]), key
        return trs

    def pre(self, k):
        return {key[len(f"l{k}/pre/"):]: self.z[key] for key in self.z.files if key.startswith(f"l{k}/pre/")}

    def mb(self, k, i):
        p = f"l{k}/mb{i}/"
        return {key[len(p):]: self.z[key] for key in self.z.files if key.startswith(p)}

    def agent_kwargs(self):
        kw = dict(state_size=self.S, action_size=self.A, hidden_size=self.H, network=self.network, optim_config={"name": "adam", "lr": self.lr}, gamma=self.gamma,
                  batch_size=self.B, n_step=self.T, n_epoch=1, _lambda=self.lam, clip_grad_norm=self.clip, run_step=100000, num_workers=self.W, lr_decay=False)
        for j, k in enumerate(NAMES):
            kw[k], kw["min_" + k], kw["eps_" + k] = self.mult0[j], self.floors[j], self.eps[j]
        return kw


def load_fixture(name):
    import os

    return Fixture(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False))
