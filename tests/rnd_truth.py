"""Float64 restatement of RND-PPO (the distillation module with its running moments and reward filter, the two advantage streams and their
mix, PPO's loss with two clipped critics) with torch on the CPU, written from the formulas: the comparator of tests/test_rnd_cpu.py and
tests/test_rnd_gpu.py (test infrastructure, not the product).  Every function takes `dtype`: torch.float64 is the truth, torch.float32 the
torch-CPU-fp32 comparator that fp64_truth's criterion |ours - fp64| <= max(1e-5, 2 |fp32 - fp64|) needs.

  module     x = clip((s' - mean) / (sqrt(var) + 1e-7), +-5); p, t = two trunks fc1 -> bn1 -> ReLU -> fc2 -> bn2 -> ReLU under BATCH
             statistics (all four batch norms advance their running statistics on every forward); r_i = mean_f (p - t)^2
  reward     the observation moments merged first, r_i over the rollout, the filter per worker, rms_ri from T copies of the FINAL filter
             state (the filter hands out its own storage, so the stack the moments see is aliased), then r_i / (sqrt(var) + 1e-7)
  update     loss = mean of the normalised r_i of a minibatch; gradients of the predictor's eight tensors only, clipped over exactly those
  gae        delta_t = r_t + f_t gamma v'_t - v_t, adv_t = delta_t + f_t gamma lambda adv_{t+1} per row of n_step, f = 1 - done (or 1)
  mix        ext adv_e + int adv_i, per row (x - mean) / (std + 1e-7) with the unbiased std
  ppo loss   actor = -mean min(ratio adv, clamp(ratio) adv), critic = max(mean (v - ret)^2, mean (v_old + clamp(v - v_old) - ret)^2) for both
             value heads, entropy = -mean H; loss = actor + vf (critic_e + critic_i) + ent entropy
plus the case builders of the sweeps and `margins_of`, the distance of a case from each discontinuity."""
from collections import OrderedDict
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

FEATURE = 256
NETS, LAYERS = ("predict", "target"), ("fc1", "fc2", "bn1", "bn2")
BN = tuple(f"{l}_{n}_mlp" for n in NETS for l in ("bn1", "bn2"))
BLOCK_KEYS = ("rms_obs.mean", "rms_obs.var", "rms_obs.count", "rms_ri.mean", "rms_ri.var", "rms_ri.count", "rff.rewems") + tuple(
    f"{b}.{s}" for b in BN for s in ("running_mean", "running_var"))
TOL = 1e-5  # the project's convention, the `tol` of fp64_truth.vs_exact


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(dtype)


def config(S, H, W=1, gamma_i=0.99, obs_norm=True, ri_norm=True, bn=True):
    return dict(S=S, H=H, W=W, gamma_i=gamma_i, obs_norm=obs_norm, ri_norm=ri_norm, bn=bn)


def shapes(cfg):
    """name -> shape of the module's weight tensors in the registration order: the four linear layers (predictor first), then the batch norms."""
    S, H = cfg["S"], cfg["H"]
    out = OrderedDict()
    for n in NETS:
        for l, sh in (("fc1", (H, S)), ("fc2", (FEATURE, H))):
            out[f"{l}_{n}_mlp.weight"], out[f"{l}_{n}_mlp.bias"] = sh, (sh[0],)
    if cfg["bn"]:
        for n in NETS:
            for l, c in (("bn1", H), ("bn2", FEATURE)):
                out[f"{l}_{n}_mlp.weight"], out[f"{l}_{n}_mlp.bias"] = (c,), (c,)
    return out


def trainable(cfg):
    return [k for k in shapes(cfg) if "predict" in k]


def random_weights(cfg, rng):
    """Linear layers uniform in +- sqrt(3 / fan_in) (unit-variance pre-activations for unit-variance inputs), batch-norm weights around 1 and
    biases around 0 -- the target's too, so that no path is hidden behind an identity."""
    out = OrderedDict()
    for k, sh in shapes(cfg).items():
        if k.startswith("bn"):
            out[k] = ((1.0 if k.endswith("weight") else 0.0) + 0.2 * rng.randn(*sh)).astype(np.float32)
        elif k.endswith("weight"):
            out[k] = (rng.uniform(-1.0, 1.0, size=sh) * np.sqrt(3.0 / sh[1])).astype(np.float32)
        else:
            out[k] = (0.1 * rng.randn(*sh)).astype(np.float32)
    return out


def fresh_block(cfg):
    S, H, W = cfg["S"], cfg["H"], cfg["W"]
    z, o = (lambda n: np.zeros(n, np.float32)), (lambda n: np.ones(n, np.float32))
    b = OrderedDict([("rms_obs.mean", z(S)), ("rms_obs.var", z(S)), ("rms_obs.count", np.float32(1e-4)), ("rms_ri.mean", z(1)), ("rms_ri.var", z(1)),
                     ("rms_ri.count", np.float32(1e-4)), ("rff.rewems", z(W))])
    for k in BN:
        n = H if k.startswith("bn1") else FEATURE
        b[k + ".running_mean"], b[k + ".running_var"] = z(n), o(n)
    return b


def random_block(cfg, rng):
    """A block as it looks after some learns: non-trivial moments, counts and filter state."""
    b = fresh_block(cfg)
    S, W = cfg["S"], cfg["W"]
    b["rms_obs.mean"] = (0.3 * rng.randn(S)).astype(np.float32)
    b["rms_obs.var"] = (0.5 + rng.rand(S)).astype(np.float32)
    b["rms_obs.count"] = np.float32(40.0001)
    b["rms_ri.mean"] = np.asarray([0.7], np.float32)
    b["rms_ri.var"] = np.asarray([0.09], np.float32)
    b["rms_ri.count"] = np.float32(24.0001)
    b["rff.rewems"] = (0.5 + rng.rand(W)).astype(np.float32)
    for k in BN:
        n = b[k + ".running_mean"].size
        b[k + ".running_mean"] = (0.1 * rng.randn(n)).astype(np.float32)
        b[k + ".running_var"] = (0.5 + rng.rand(n)).astype(np.float32)
    return b


# ---------------------------------------------------------------------------------- running moments and the filter
def moments_merge(mean, var, count, x, dtype=torch.float64):
    """Parallel-variance merge of a batch x [n, ...] (mean, UNBIASED variance, n) into (mean, var, count)."""
    mean, var, count, x = _t(mean, dtype), _t(var, dtype), _t(count, dtype), _t(x, dtype)
    n = x.shape[0]
    b_mean, b_var = x.mean(0), x.var(0, unbiased=True)
    delta, tot = b_mean - mean, count + n
    m2 = var * count + b_var * n + delta ** 2 * count * n / tot
    return mean + delta * n / tot, m2 / tot, n + count


def filter_final(rewems, r_wt, gamma, dtype=torch.float64):
    """The filter's state after the T steps of r_wt [W, T]: rewems <- rewems gamma + r_t."""
    rew, r = _t(rewems, dtype), _t(r_wt, dtype)
    for t in range(r.shape[1]):
        rew = rew * gamma + r[:, t]
    return rew


# ---------------------------------------------------------------------------------- the module
def _params(weights, dtype, cfg, grad):
    return OrderedDict((k, _t(v, dtype).clone().requires_grad_(grad and k in trainable(cfg))) for k, v in weights.items())


def normalize_obs(x, blk, dtype):
    return torch.clip((x - _t(blk["rms_obs.mean"], dtype)) / (torch.sqrt(_t(blk["rms_obs.var"], dtype)) + 1e-7), min=-5.0, max=5.0)


def forward(cfg, P, blk, s2, dtype=torch.float64):
    """-> dict(r_raw [b], p, t, x, z1 / z2: {net: pre-activation input of bn1 / bn2}, u1 / u2: {net: the ReLU's input}, run: the running statistics after)."""
    x = _t(s2, dtype)
    if cfg["obs_norm"]:
        x = normalize_obs(x, blk, dtype)
    run = {k: _t(blk[k], dtype).clone() for k in BLOCK_KEYS if k.startswith("bn")}
    out = dict(x=x, z1={}, z2={}, u1={}, u2={}, run=run)
    feat = {}
    for n in NETS:
        lin = lambda name, v: F.linear(v, P[f"{name}_{n}_mlp.weight"], P[f"{name}_{n}_mlp.bias"])
        bn = (lambda name, v: F.batch_norm(v, run[f"{name}_{n}_mlp.running_mean"], run[f"{name}_{n}_mlp.running_var"], P[f"{name}_{n}_mlp.weight"],
                                           P[f"{name}_{n}_mlp.bias"], True, 0.1, 1e-5)) if cfg["bn"] else (lambda name, v: v)
        out["z1"][n] = lin("fc1", x)
        out["u1"][n] = bn("bn1", out["z1"][n])
        out["z2"][n] = lin("fc2", F.relu(out["u1"][n]))
        out["u2"][n] = bn("bn2", out["z2"][n])
        feat[n] = F.relu(out["u2"][n])
    out["p"], out["t"] = feat["predict"], feat["target"]
    out["r_raw"] = torch.mean((out["p"] - out["t"]) ** 2, dim=1)
    return out


def reward_pass(cfg, weights, blk, s2, dtype=torch.float64):
    """The pre-pass on the module: observation moments, r_i, filter, rms_ri, normalisation.  -> dict(r_raw, r_i, r_i_mean, block, x, u1, u2)."""
    with torch.no_grad():
        nb = OrderedDict((k, _t(v, dtype)) for k, v in blk.items())
        nb["rms_obs.mean"], nb["rms_obs.var"], nb["rms_obs.count"] = moments_merge(blk["rms_obs.mean"], blk["rms_obs.var"], blk["rms_obs.count"], s2, dtype)
        out = forward(cfg, _params(weights, dtype, cfg, False), nb, s2, dtype)
        W = cfg["W"]
        r_wt = out["r_raw"].reshape(W, -1)
        T = r_wt.shape[1]
        final = filter_final(blk["rff.rewems"], r_wt, cfg["gamma_i"], dtype)
        nb["rff.rewems"] = final
        stack = final.unsqueeze(0).expand(T, -1).reshape(-1, 1)  # T copies of the FINAL state
        nb["rms_ri.mean"], nb["rms_ri.var"], nb["rms_ri.count"] = moments_merge(blk["rms_ri.mean"], blk["rms_ri.var"], blk["rms_ri.count"], stack, dtype)
        r_i = out["r_raw"] / (torch.sqrt(nb["rms_ri.var"]) + 1e-7) if cfg["ri_norm"] else out["r_raw"]
        nb.update(out["run"])
        return dict(r_raw=out["r_raw"], r_i=r_i, r_i_mean=r_i.mean(), block=nb, x=out["x"], u1=out["u1"], u2=out["u2"])


def clip_(grads, max_norm):
    """Global-norm clip of a dict of gradients, in place; -> the total norm."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).to(next(iter(grads.values())).dtype)
    if max_norm:
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        for g in grads.values():
            g.mul_(coef)
    return total


def update(cfg, weights, blk, s2, max_norm=None, dtype=torch.float64):
    """One minibatch.  -> dict(loss, grads {trainable name: raw}, clipped, norm, run, x, u1, u2)."""
    P = _params(weights, dtype, cfg, True)
    out = forward(cfg, P, blk, s2, dtype)
    r_i = out["r_raw"] / (torch.sqrt(_t(blk["rms_ri.var"], dtype)) + 1e-7) if cfg["ri_norm"] else out["r_raw"]
    loss = r_i.mean()
    loss.backward()
    grads = OrderedDict((k, P[k].grad.detach().clone()) for k in trainable(cfg))
    clipped = OrderedDict((k, g.clone()) for k, g in grads.items())
    norm = clip_(clipped, max_norm)
    return dict(loss=loss.detach(), grads=grads, clipped=clipped, norm=norm, run=out["run"], x=out["x"].detach(),
                u1={n: v.detach() for n, v in out["u1"].items()}, u2={n: v.detach() for n, v in out["u2"].items()})


# ---------------------------------------------------------------------------------- advantages
def gae(reward, done, value, next_value, n_step, gamma, lam, episodic=True, dtype=torch.float64):
    """-> (adv [M], ret [M]), rows of n_step; episodic False: the factor (1 - done) is 1 in the delta and in the scan."""
    r, d, v, vn = (_t(a, dtype).reshape(-1, n_step) for a in (reward, done, value, next_value))
    f = (1 - d) if episodic else torch.ones_like(d)
    adv = r + f * gamma * vn - v
    for t in reversed(range(n_step - 1)):
        adv[:, t] = adv[:, t] + f[:, t] * gamma * lam * adv[:, t + 1]
    return adv.reshape(-1), (adv + v).reshape(-1)


def adv_mix(adv_e, adv_i, n_step, ext, intr, standardize, dtype=torch.float64):
    a = (ext * _t(adv_e, dtype) + intr * _t(adv_i, dtype)).reshape(-1, n_step)
    if standardize:
        a = (a - a.mean(1, keepdim=True)) / (a.std(1, keepdim=True, unbiased=True) + 1e-7)
    return a.reshape(-1)


# ---------------------------------------------------------------------------------- PPO's loss with two critics
def ppo_loss(cont, heads, A, action, adv, ret, ret_i, v_old, vi_old, lp_old, eps, vf, ent, dtype=torch.float64):
    """heads [B, >= nA + 2] = (head0 | head1 | v | v_i | ...), the other arguments the minibatch's rows.  -> dict(stats: actor, critic_e,
    critic_i, entropy, max_ratio, min_prob, loss; grad [B, nA + 2]; rows: ratio, dv, dvi; means: c1, c2, i1, i2)."""
    nv = 2 * A if cont else A
    h = _t(heads, dtype)[:, : nv + 2].clone().requires_grad_(True)
    action, adv, ret, ret_i, v_old, vi_old, lp_old = (_t(a, dtype) for a in (action, adv, ret, ret_i, v_old, vi_old, lp_old))
    B = h.shape[0]
    if cont:
        mu, std = torch.clamp(h[:, :A], -5.0, 5.0), torch.exp(torch.tanh(h[:, A : 2 * A]))
        one = torch.tensor(1 - 1e-7, dtype=torch.float32).to(dtype)  # the clamp is applied to a float32 action tensor
        z = torch.atanh(torch.clamp(action.reshape(B, A), -one, one))
        lp = -((z - mu) ** 2) / (2 * std ** 2) - torch.log(std) - 0.5 * np.log(2 * np.pi)
        H = 0.5 + 0.5 * np.log(2 * np.pi) + torch.log(std)
        ratio = torch.exp((lp - lp_old.reshape(B, A)).sum(1))
    else:
        logp = F.log_softmax(h[:, :A], dim=1)
        lp = logp.gather(1, action.reshape(B, 1).long())
        H = -(logp.exp() * logp).sum(1)
        ratio = torch.exp((lp - lp_old.reshape(B, 1)).sum(1))
    adv = adv.reshape(B)
    actor = -torch.min(ratio * adv, torch.clamp(ratio, 1 - eps, 1 + eps) * adv).mean()
    crit, means, dvs = [], [], []
    for col, r, old in ((nv, ret, v_old), (nv + 1, ret_i, vi_old)):
        v, r, old = h[:, col], r.reshape(B), old.reshape(B)
        c1, c2 = ((v - r) ** 2).mean(), ((old + torch.clamp(v - old, -eps, eps) - r) ** 2).mean()
        crit.append(torch.max(c1, c2))
        means += [float(c1.detach()), float(c2.detach())]
        dvs.append((v - old).detach())
    entropy = -H.mean()
    loss = actor + vf * (crit[0] + crit[1]) + ent * entropy
    loss.backward()
    stats = dict(actor=float(actor), critic_e=float(crit[0]), critic_i=float(crit[1]), entropy=float(entropy), max_ratio=float(ratio.max()), min_prob=float(lp.exp().min()),
                 loss=float(loss))
    return dict(stats=stats, grad=h.grad.detach(), rows=dict(ratio=ratio.detach(), dv=dvs[0], dvi=dvs[1]), means=dict(zip(("c1", "c2", "i1", "i2"), means)))


# ---------------------------------------------------------------------------------- cases
def rollout(cfg, rows, rng):
    """next_state of `rows` transitions: observations on different scales per feature, a few beyond the clip."""
    S = cfg["S"]
    scale = (0.5 + 2.0 * rng.rand(S)).astype(np.float32)
    s2 = (rng.randn(rows, S) * scale).astype(np.float32)
    s2[rng.rand(rows, S) < 0.02] *= 8.0
    return s2


UPDATE_ROWS = (2, 3, 15, 16, 17, 63, 64, 65, 257)
UPDATE_S = (2, 4, 11)
UPDATE_H = (16, 32, 512)
REWARD_W, REWARD_T = (1, 2, 8), (1, 2, 9)
MIX_WT = ((1, 2), (2, 8), (8, 128), (3, 65))
LOSS_ROWS = (1, 2, 63, 64, 65, 256, 1024)
LOSS_A = {False: (2, 3, 6), True: (1, 3, 17)}
LOSS_VARIANTS = ("plain", "clipped", "critic")


# Seeds.  A case's generator is seeded by its tag; where that draw lands within CLEAR (below) of a discontinuity the tag gets the first salt
# that does not -- found with the float64 truth alone, checked by tests/test_rnd_cpu.py::test_no_sweep_case_sits_on_a_discontinuity
SALT = {"plain_b65": 1, "plain_S11_H32": 1}


def _rng(tag):
    salt = SALT.get(tag, 0)
    return np.random.RandomState(zlib.crc32((tag if not salt else f"{tag}#{salt}").encode()) % (1 << 31))


def cases():
    """(tag, cfg, b) of the update sweep: every b at the base shape, every S and H at b = 17 and 64, each with batch norm on and off (one row
    needs it off)."""
    out = []
    for bn in (True, False):
        t = "" if bn else "plain_"
        for b in UPDATE_ROWS:
            out.append((f"{t}b{b}", config(4, 32, bn=bn, obs_norm=bn, ri_norm=bn), b))
        for S in UPDATE_S:
            for H in UPDATE_H:
                if (S, H) != (4, 32):
                    out.append((f"{t}S{S}_H{H}", config(S, H, bn=bn), 17 if H == 512 else 64))
    return out


def reward_cases():
    """(tag, cfg, M): W x T with W T >= 2 with every switch on, and each switch off in turn at W 2, T 9."""
    out = [(f"W{W}_T{T}", config(4, 32, W=W), W * T) for W in REWARD_W for T in REWARD_T if W * T >= 2]
    for k in ("obs_norm", "ri_norm", "bn"):
        out.append((f"no_{k}", config(4, 32, W=2, **{k: False}), 18))
    return out


def case_inputs(tag, cfg, rows):
    """(weights, block, next_state) of a case, from a generator seeded by the tag (the same in every process)."""
    rng = _rng(tag)
    return random_weights(cfg, rng), random_block(cfg, rng), rollout(cfg, rows, rng)


def update_case(tag, cfg, b):
    """An update case: a rollout of b + 7 rows and the index list that picks its b rows.  -> (weights, block, next_state, idx)"""
    w, blk, s2 = case_inputs(tag, cfg, b + 7)
    return w, blk, s2, np.random.RandomState(b).permutation(b + 7)[:b].astype(np.int64)


def loss_cases():
    out = []
    for cont in (False, True):
        for A in LOSS_A[cont]:
            for b in LOSS_ROWS:
                for variant in LOSS_VARIANTS:
                    out.append((f"{'cont' if cont else 'disc'}_A{A}_b{b}_{variant}", cont, A, b, variant))
    return out


def loss_case(tag, cont, A, b, variant):
    """Inputs of one loss case.  plain: ratios on both sides of the clip, small value moves; clipped: log pi_old shifted so that EVERY ratio
    leaves [1 - eps, 1 + eps]; critic: the stored values far from the predictions, so that for both heads the clipped mean is the larger.
    -> dict(heads [b, ld], action, adv, ret, ret_i, v_old, vi_old, lp_old, eps, vf, ent, ld)"""
    rng = _rng(tag)
    nv = 2 * A if cont else A
    ld = nv + 2 + (b % 3)  # padding columns of 0, 1, 2
    heads = rng.randn(b, ld).astype(np.float32)
    if cont:
        heads[:, :A] *= 2.0
        if b >= 2:
            heads[0, 0], heads[1, 0] = 6.5, -7.25  # a clamped mu on each side
        action = np.tanh(rng.randn(b, A)).astype(np.float32)
        action[0, -1] = 1.0  # a saturated action
    else:
        action = rng.randint(0, A, size=(b, 1)).astype(np.float32)
    heads[:, nv:nv + 2] = rng.randn(b, 2).astype(np.float32)
    adv = rng.randn(b).astype(np.float32)
    eps = 0.1
    h64 = torch.from_numpy(heads.astype(np.float64))
    if cont:
        mu, std = torch.clamp(h64[:, :A], -5, 5), torch.exp(torch.tanh(h64[:, A:2 * A]))
        one = float(np.float32(1 - 1e-7))
        z = torch.atanh(torch.clamp(torch.from_numpy(action.astype(np.float64)), -one, one))
        lp = (-((z - mu) ** 2) / (2 * std ** 2) - torch.log(std) - 0.5 * np.log(2 * np.pi)).numpy()
    else:
        lp = F.log_softmax(h64[:, :A], 1).gather(1, torch.from_numpy(action).long()).numpy()
    width = lp.shape[1]
    if variant == "clipped":
        shift = np.where(rng.rand(b, 1) < 0.5, -1.0, 1.0) * (0.3 + 0.3 * rng.rand(b, 1))  # |log ratio| in [0.3, 0.6]: outside log(1 +- 0.1)
    else:
        shift = 0.25 * rng.randn(b, 1)
        shift[np.abs(np.abs(shift) - 0.1) < 0.02] = 0.05  # away from the clip edge
    lp_old = (lp - shift / width).astype(np.float32)
    v, vi = heads[:, nv], heads[:, nv + 1]
    if variant == "critic":
        # the stored value between the prediction and the return, further than eps from the prediction: the clipped prediction stays further from
        # the return than the plain one, so the clipped mean is the larger
        ret, ret_i = (v + 3.0 + rng.rand(b)).astype(np.float32), (vi - 3.0 - rng.rand(b)).astype(np.float32)
        v_old, vi_old = (v - 0.5 - rng.rand(b)).astype(np.float32), (vi + 0.5 + rng.rand(b)).astype(np.float32)
    else:
        ret, ret_i = (v + rng.randn(b)).astype(np.float32), (vi + rng.randn(b)).astype(np.float32)
        dv, dvi = 0.2 * rng.randn(b), 0.2 * rng.randn(b)
        dv[np.abs(np.abs(dv) - eps) < 0.01] = 0.03
        dvi[np.abs(np.abs(dvi) - eps) < 0.01] = 0.03
        dv[0], dvi[0] = 0.25, -0.3  # one row outside the value clip, so that the two means of a head differ whatever b is
        v_old, vi_old = (v - dv).astype(np.float32), (vi - dvi).astype(np.float32)
    return dict(heads=heads, action=action, adv=adv, ret=ret, ret_i=ret_i, v_old=v_old, vi_old=vi_old, lp_old=lp_old, eps=eps, vf=0.5, ent=0.01, ld=ld)


def mix_case(W, T, seed=0):
    rng = np.random.RandomState(1000 * W + T + seed)
    M = W * T
    g = lambda: rng.randn(M).astype(np.float32)
    return dict(reward=g(), r_i=np.abs(g()), done=(rng.rand(M) < 0.1).astype(np.float32), v=g(), vn=g(), vi=g(), vin=g())


# ---------------------------------------------------------------------------------- distance from the discontinuities
def module_margins(out):
    """Smallest distance of a case of the module from a kink: a ReLU input at 0 (relative to the layer's root mean square, the size of the
    terms whose float32 rounding could move it), a normalised observation at +-5."""
    pre = min(float(v.abs().min()) / float((v ** 2).mean().sqrt()) for d in (out["u1"], out["u2"]) for v in d.values())
    obs = float((out["x"].abs() - 5.0).abs()[out["x"].abs() < 5.0].min()) if bool((out["x"].abs() < 5.0).any()) else 1.0
    return dict(pre_activation=pre, obs_clip=obs)


def loss_margins(res, eps):
    """Smallest distance of a loss case from a kink: ratio at 1 +- eps, v - v_old at +- eps (both heads), the two critic means of a head equal."""
    r, m = res["rows"], res["means"]
    edge = lambda x, c: float((x - c).abs().min())
    return dict(ratio=min(edge(r["ratio"], 1 - eps), edge(r["ratio"], 1 + eps)), dv=min(edge(r["dv"].abs(), eps), edge(r["dvi"].abs(), eps)),
                critic=min(abs(m["c1"] - m["c2"]) / max(m["c1"], m["c2"]), abs(m["i1"] - m["i2"]) / max(m["i1"], m["i2"])))


# a case counts as clear of a kink when it is further from it than float32 arithmetic can move it: 1e-4 in the quantities of order one
# (ratio, value move, relative difference of the means, normalised observation), 1e-6 of the layer's root-mean-square pre-activation
CLEAR = dict(ratio=1e-4, dv=1e-4, critic=1e-4, obs_clip=1e-4, pre_activation=1e-6)


def rel(ours, exact):
    """max |ours - exact| relative to max |exact|."""
    exact = np.asarray(exact.detach().cpu() if torch.is_tensor(exact) else exact, dtype=np.float64)
    ours = np.asarray(ours.detach().cpu() if torch.is_tensor(ours) else ours, dtype=np.float64).reshape(exact.shape)
    return float(np.abs(ours - exact).max()) / (float(np.abs(exact).max()) + 1e-30)


# ---------------------------------------------------------------------------------- the policy-value net with two value heads
def policy_heads(P, x, cont):
    """head.l -> ReLU -> l -> ReLU -> the raw heads stacked as the library keeps them: (pi | v | v_i) or (mu | log_std | v | v_i)."""
    lin = lambda name, v: F.linear(v, P[name + ".weight"], P[name + ".bias"])
    h = F.relu(lin("l", F.relu(lin("head.l", x))))
    return torch.cat([lin(k, h) for k in ((("mu", "log_std") if cont else ("pi",)) + ("v", "v_i"))], 1)


def log_prob(cont, heads, A, action, dtype):
    """log pi(action) per row [b, 1] (discrete) or per dimension [b, A] (continuous)."""
    h, action = _t(heads, dtype), _t(action, dtype)
    if cont:
        mu, std = torch.clamp(h[:, :A], -5.0, 5.0), torch.exp(torch.tanh(h[:, A : 2 * A]))
        one = torch.tensor(1 - 1e-7, dtype=torch.float32).to(dtype)
        z = torch.atanh(torch.clamp(action, -one, one))
        return -((z - mu) ** 2) / (2 * std ** 2) - torch.log(std) - 0.5 * np.log(2 * np.pi)
    return F.log_softmax(h[:, :A], 1).gather(1, action.long())


# ---------------------------------------------------------------------------------- fixtures of tools/gen_golden_rnd.py
FIXTURES = ("rnd_discrete", "rnd_continuous", "rnd_plain", "rnd_cartpole")
SMALL = FIXTURES[:3]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GAMMA, LAMBDA, CLIP, EPS_CLIP, GAMMA_I, EXT, INT = 0.99, 0.95, 1.0, 0.1, 0.99, 2.0, 1.0
# B 6: minibatches of 6, 6 and 4.  The ragged one is kept above three rows on purpose: over a batch norm of two rows the REFERENCE's own float32
# gradients are 6e-5 to 1.2e-4 of their largest entry from float64 (the sweep's b2 case, torch on the CPU, by thread count), more than the
# fixture tolerance, so a record there pins torch's rounding and not the algorithm; two and three rows are the float64 sweep's (b2, b3)
_SMALL = dict(H=32, W=2, T=8, B=6, lr=3e-3, n_epoch=1, learns=2, recipe=False, thin_limit=4096, vf=0.5, ent=0.01)
SPECS = {
    "rnd_discrete": dict(_SMALL, S=4, A=3, cont=False, on=True, non_episodic=False, std=False, non_extrinsic=False),
    "rnd_continuous": dict(_SMALL, S=5, A=2, cont=True, on=True, non_episodic=True, std=True, non_extrinsic=False),
    "rnd_plain": dict(_SMALL, S=4, A=3, cont=False, on=False, non_episodic=False, std=False, non_extrinsic=True),
    "rnd_cartpole": dict(S=4, A=2, H=512, W=8, T=128, B=64, cont=False, lr=1e-4, n_epoch=3, on=True, learns=2, recipe=True, thin_limit=4096, vf=0.5, ent=0.01,
                         non_episodic=False, std=False, non_extrinsic=False),  # config/rnd_ppo/cartpole.py
}
CURVE_CONFIG = dict(workers=8, n_step=128, iterations=40, seeds=(1, 2, 3), run_step=100000,
                    agent=dict(state_size=4, action_size=2, hidden_size=512, network="discrete_policy_separate_value", head="mlp", optim_config={"name": "adam", "lr": 1e-4},
                               gamma=0.99, batch_size=64, n_step=128, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, vf_coef=0.5, ent_coef=0.01, clip_grad_norm=1.0,
                               use_standardization=False, lr_decay=True, rnd_network="rnd_mlp", gamma_i=0.99, extrinsic_coeff=2.0, intrinsic_coeff=1.0,
                               obs_normalize=True, ri_normalize=True, batch_norm=True, non_episodic=False))  # config/rnd_ppo/cartpole.py


def agent_kwargs(spec):
    """The constructor arguments of a fixture's agent, the reference's and ours alike (without `device`)."""
    return dict(state_size=spec["S"], action_size=spec["A"], hidden_size=spec["H"],
                network="continuous_policy_separate_value" if spec["cont"] else "discrete_policy_separate_value", head="mlp", optim_config={"name": "adam", "lr": spec["lr"]},
                gamma=GAMMA, batch_size=spec["B"], n_step=spec["T"], n_epoch=spec["n_epoch"], _lambda=LAMBDA, epsilon_clip=EPS_CLIP, vf_coef=spec["vf"], ent_coef=spec["ent"],
                clip_grad_norm=CLIP, use_standardization=spec["std"], run_step=100000, num_workers=spec["W"], lr_decay=False, rnd_network="rnd_mlp", gamma_i=GAMMA_I,
                extrinsic_coeff=EXT, intrinsic_coeff=INT, obs_normalize=spec["on"], ri_normalize=spec["on"], batch_norm=spec["on"], non_episodic=spec["non_episodic"],
                non_extrinsic=spec["non_extrinsic"])


def curve_end(curve):
    """The last iterations' mean episode length: the mean of the last five iterations."""
    return float(np.mean(curve[-5:]))


def curve_criterion(ref):
    """(the reference's end, the margin) of the curve test from the reference's own seeds as the fixture records them: the mean of the seeds'
    ends, and their spread (the largest end minus the smallest)."""
    ends = [curve_end(c) for c in ref]
    return float(np.mean(ends)), float(max(ends) - min(ends))


def rnd_recipe(named_shapes, seed):
    """Recipe weights of the module's weight tensors (oracle.synth's streams, keyed by "rnd." + name): linear layers as synth draws them, batch
    norm weights 1 + a draw in +-0.1, biases a draw in +-0.1."""
    from oracle import synth

    out = OrderedDict()
    for k, sh in named_shapes.items():
        v = synth.recipe_tensor("rnd." + k, tuple(sh), seed)
        out[k] = np.ascontiguousarray(v + (1.0 if (k.startswith("bn") and k.endswith("weight")) else 0.0), dtype=np.float32)
    return out


class Fixture:
    """One fixture file: the spec, the rollouts, the starting state_dicts of both networks (stored, or regenerated from the recipe and checked
    against the stored sample) and per learn `l<k>/` what the reference computed."""

    def __init__(self, name):
        from oracle import synth

        self.name, self.spec = name, SPECS[name]
        self.z = z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
        g = lambda k: z[f"hyper/{k}"].item()
        sp = self.spec
        for k in ("S", "A", "H", "W", "T", "B", "n_epoch", "learns"):
            assert int(g(k)) == sp[k], f"{name}: the fixture was generated for another {k}: rerun tools/gen_golden_rnd.py"
        self.S, self.A, self.H, self.W, self.T, self.B, self.cont, self.lr = sp["S"], sp["A"], sp["H"], sp["W"], sp["T"], sp["B"], sp["cont"], sp["lr"]
        self.M, self.limit, self.recipe, self.learns, self.init_seed = self.W * self.T, int(g("thin_limit")), bool(int(g("recipe"))), sp["learns"], int(g("init_seed"))
        self.cfg = config(self.S, self.H, W=self.W, gamma_i=GAMMA_I, obs_norm=sp["on"], ri_norm=sp["on"], bn=sp["on"])
        names = [k[len("sd0/"):] for k in z.files if k.startswith("sd0/")]
        rnames = [k[len("rnd0/"):] for k in z.files if k.startswith("rnd0/")]
        if self.recipe:
            sd = synth.ppo_recipe(OrderedDict((k, tuple(int(s) for s in z[f"shape/{k}"])) for k in names), int(g("recipe_seed")))
            tr = rnd_recipe(OrderedDict((k, tuple(int(s) for s in z[f"shape/rnd.{k}"])) for k in rnames if k in shapes(self.cfg)), int(g("recipe_seed")))
            for k in names:
                assert np.array_equal(self.thin(sd[k]), z[f"sd0/{k}"]), k
            for k in tr:
                assert np.array_equal(self.thin(tr[k]), z[f"rnd0/{k}"]), k
            self.sd0 = OrderedDict((k, sd[k]) for k in names)
            self.rnd0 = OrderedDict((k, tr[k] if k in tr else z[f"rnd0/{k}"]) for k in rnames)
        else:
            self.sd0 = OrderedDict((k, z[f"sd0/{k}"]) for k in names)
            self.rnd0 = OrderedDict((k, z[f"rnd0/{k}"]) for k in rnames)

    def thin(self, a):
        from oracle import synth

        a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
        return synth.thin(a, self.limit) if self.limit else a

    def n_minibatch(self):
        return self.spec["n_epoch"] * ((self.M + self.B - 1) // self.B)

    def rollout(self, k):
        """The transitions of learn k as the list of dicts process() takes."""
        from oracle import synth

        z, p = self.z, f"l{k}/in_"
        if p + "state" in z.files:
            return [{key: z[p + key][i : i + 1] for key in ("state", "action", "reward", "next_state", "done")} for i in range(self.M)]
        trs = synth.ppo_rollout(np.random.RandomState(int(z[f"l{k}/rollout_seed"])), self.M, self.S, self.A, self.cont, clamp_every=5 if self.cont else 0)
        for key in ("state", "reward", "action"):
            got = synth.row_checksum(np.concatenate([t[key] for t in trs], 0).astype(np.float32))[:: max(1, self.M // 64)]
            assert np.array_equal(got, z[f"{p}{key}_check"]), key
        return trs

    def cols(self, k):
        trs = self.rollout(k)
        return {key: np.concatenate([t[key] for t in trs], 0).astype(np.float32) for key in ("state", "action", "next_state", "reward", "done")}

    def sub(self, prefix):
        return OrderedDict((key[len(prefix):], self.z[key]) for key in self.z.files if key.startswith(prefix))


def load_fixture(name):
    return Fixture(name)


def learn_truth(fx, k, state, dtype=torch.float64):
    """One learn of a fixture on the truth: the pre-pass, then every minibatch (the fixture's index lists) with both Adams.  `state`: dict(P,
    R: the two networks' parameters as torch Parameters of `dtype`, blk, opt, ropt), advanced IN PLACE.  -> dict(pre: r_i, value, v_i, adv, ret,
    ret_i, log_prob_old; mb: per minibatch dict(actor_loss, critic_e_loss, critic_i_loss, entropy_loss, rnd_loss, grad, rnd_grad))."""
    sp, cfg, cont, A, T = fx.spec, fx.cfg, fx.cont, fx.A, fx.T
    c = fx.cols(k)
    P, R = state["P"], state["R"]
    det = lambda d: OrderedDict((kk, p.detach()) for kk, p in d.items())
    rp = reward_pass(cfg, det(R), state["blk"], c["next_state"], dtype)
    state["blk"] = {kk: np.asarray(v.detach().double()) for kk, v in rp["block"].items()}
    with torch.no_grad():
        h, hn = policy_heads(P, _t(c["state"], dtype), cont), policy_heads(P, _t(c["next_state"], dtype), cont)
    nv = 2 * A if cont else A
    lp_old = log_prob(cont, h, A, c["action"], dtype)
    reward = np.zeros_like(c["reward"]) if sp["non_extrinsic"] else c["reward"]
    adv_e, ret = gae(reward, c["done"], h[:, nv], hn[:, nv], T, GAMMA, LAMBDA, True, dtype)
    adv_i, ret_i = gae(rp["r_i"], c["done"], h[:, nv + 1], hn[:, nv + 1], T, GAMMA_I, LAMBDA, not sp["non_episodic"], dtype)
    adv = adv_mix(adv_e, adv_i, T, EXT, INT, sp["std"], dtype)
    out = dict(pre=dict(r_i=rp["r_i"], value=h[:, nv], v_i=h[:, nv + 1], adv=adv, ret=ret, ret_i=ret_i, log_prob_old=lp_old.reshape(-1)), mb=[])
    for i in range(fx.n_minibatch()):
        idx = torch.from_numpy(np.asarray(fx.z[f"l{k}/mb{i}/idx"]).astype(np.int64))
        for p in P.values():
            p.grad = None
        heads = policy_heads(P, _t(c["state"], dtype)[idx], cont)
        res = ppo_loss(cont, heads.detach(), A, c["action"][idx], adv[idx], ret[idx], ret_i[idx], h[idx, nv], h[idx, nv + 1], lp_old[idx], EPS_CLIP, sp["vf"], sp["ent"], dtype)
        heads.backward(res["grad"])
        grads = OrderedDict((kk, p.grad.detach().clone()) for kk, p in P.items())
        clip_(grads, CLIP)
        for kk, p in P.items():
            p.grad = grads[kk].clone()
        state["opt"].step()
        u = update(cfg, det(R), state["blk"], c["next_state"][idx], CLIP, dtype)
        for kk, p in R.items():
            p.grad = u["clipped"][kk].reshape(p.shape).clone() if kk in u["clipped"] else None
        state["ropt"].step()
        for kk, v in u["run"].items():
            state["blk"][kk] = np.asarray(v.detach().double())
        s = res["stats"]
        out["mb"].append(dict(actor_loss=s["actor"], critic_e_loss=s["critic_e"], critic_i_loss=s["critic_i"], entropy_loss=s["entropy"], rnd_loss=float(u["loss"]),
                              grad=grads, rnd_grad=u["clipped"]))
    return out


def truth_state(fx, dtype=torch.float64):
    """The starting state of learn_truth from a fixture's starting state_dicts."""
    P = OrderedDict((k, torch.nn.Parameter(_t(v, dtype))) for k, v in fx.sd0.items())
    R = OrderedDict((k, torch.nn.Parameter(_t(fx.rnd0[k], dtype), requires_grad=k in trainable(fx.cfg))) for k in shapes(fx.cfg))
    blk = fresh_block(fx.cfg)
    for k in BLOCK_KEYS:
        if k in fx.rnd0:
            blk[k] = np.asarray(fx.rnd0[k])
    return dict(P=P, R=R, blk=blk, opt=torch.optim.Adam(list(P.values()), lr=fx.lr), ropt=torch.optim.Adam([p for p in R.values() if p.requires_grad], lr=fx.lr))
