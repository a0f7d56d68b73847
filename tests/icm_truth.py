"""Float64 restatement of ICM-PPO's curiosity module (core/agent/icm_ppo.py:96-102, 177-199 on core/network/icm.py:8-34, 99-218,
core/network/utils.py:6-52 and core/network/rnd.py:9-10) with torch on the CPU: the comparator of tests/test_icm_cpu.py and
tests/test_icm_gpu.py (test infrastructure, not the product).  Every function takes `dtype`: torch.float64 is the truth, torch.float32 the
torch-CPU-fp32 comparator, i.e. the reference's own arithmetic.

  moments_merge     RunningMeanStd.update: per-feature mean and UNBIASED variance of a batch merged into (mean, var, count)
  filter_states     RewardForwardFilter over a rollout as the reference REALLY behaves: `update` returns the Parameter itself, so the stack
                    the reference hands to rms_ri is T copies of the FINAL state (aliased_stack), not the sequence of states (true_stack)
  features / heads  the trunk (batch norm under batch statistics, ELU), the forward and the inverse model, both losses, raw r_i
  reward_pass       icm_ppo.py:98-102: observation moments, r_i, filter, rms_ri, normalisation, the mixed reward
  update            one minibatch: losses, parameter gradients raw and clipped, the running statistics after it
and the case builders of the kernel tests.

Tolerances.  The project's convention is rtol 1e-5 on losses and 1e-5 of a segment's largest entry on gradients, which holds wherever the
float32 comparator itself stays within half of that against float64; where it does not, the bound is four times the comparator's measured
error (four: the MFMA tiles sum in another order than torch's CPU loops).  E_REF below holds the comparator's LARGEST measured error per
quantity over update_case() of cases() and case_inputs() of reward_cases() -- the very inputs the GPU test uses -- (tests/test_icm_cpu.py
re-measures them); bound(q) is 1e-5 where E_REF[q] <= 0.5e-5, else 4 * E_REF[q]."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

FEATURE = 256
SEG = ("fc1", "fc2", "forward_fc1", "forward_fc2", "inverse_fc1", "inverse_fc2", "bn1", "bn2", "bn1_next")
BLOCK_KEYS = ("rms_obs.mean", "rms_obs.var", "rms_obs.count", "rms_ri.mean", "rms_ri.var", "rms_ri.count", "rff.rewems", "bn1.running_mean", "bn1.running_var",
              "bn2.running_mean", "bn2.running_var", "bn1_next.running_mean", "bn1_next.running_var")

# the float32 comparator's largest error against float64 over cases() (relative: losses and r_i to the value, gradients to the segment's
# largest entry, block entries to the entry's largest value), measured on the CPU by tests/test_icm_cpu.py::test_comparator_errors_are_the_recorded_ones
E_REF = {
    "loss": 2.1e-7,      # l_f, l_i (measured 2.03e-7, case b3)
    "grad": 6.8e-6,      # every segment of every case with more than three rows under batch norm, and of the cases without (measured 6.74e-6: case b63,
                         # inverse_fc2.bias, whose two entries are sums of 63 terms that nearly cancel; the next is 1.64e-6, case b17, bn1.bias)
    "grad_b2": 2.57e-4,  # batch norm over TWO rows: xhat = +-1 / sqrt(1 + eps / var), a division by the variance of two values (measured 2.57e-4, fc2.bias)
    "grad_b3": 5.4e-5,   # batch norm over THREE rows (measured 5.33e-5, fc2.weight)
    "r_i": 4.5e-7,       # raw and normalised intrinsic reward, the mixed reward (measured 4.45e-7, case W8_T128)
    "block": 7.4e-7,     # every entry of the statistics block after a call (measured 7.38e-7, case W8_T128)
}


def bound(q):
    """The convention (1e-5) where the comparator stays within half of it, else four times the comparator's error."""
    return 1e-5 if E_REF[q] <= 0.5e-5 else 4.0 * E_REF[q]


def grad_class(cfg, rows):
    return f"grad_b{rows}" if (cfg["bn"] and rows in (2, 3)) else "grad"


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(dtype)


def config(S, A, H, cont, W=1, gamma=0.99, eta=0.1, obs_norm=True, ri_norm=True, bn=True):
    return dict(S=S, A=A, H=H, cont=bool(cont), W=W, gamma=gamma, eta=eta, obs_norm=obs_norm, ri_norm=ri_norm, bn=bn)


def shapes(cfg):
    """name -> shape of every trainable tensor in the reference's registration order (icm.py:183-188)."""
    S, A, H, a = cfg["S"], cfg["A"], cfg["H"], (cfg["A"] if cfg["cont"] else 1)
    lin = OrderedDict([("fc1", (H, S)), ("fc2", (FEATURE, H)), ("forward_fc1", (H, FEATURE + a)), ("forward_fc2", (FEATURE, H + a)),
                       ("inverse_fc1", (H, 2 * FEATURE)), ("inverse_fc2", (A, H))])
    out = OrderedDict()
    for k, sh in lin.items():
        out[k + ".weight"], out[k + ".bias"] = sh, (sh[0],)
    if cfg["bn"]:
        for k, c in (("bn1", H), ("bn2", FEATURE), ("bn1_next", H)):
            out[k + ".weight"], out[k + ".bias"] = (c,), (c,)
    return out


def random_weights(cfg, rng):
    """Linear layers at torch's default scale (uniform +- 1 / sqrt(fan_in)), batch-norm weights around 1 and biases around 0: perturbed, so that
    no gradient path is hidden behind an identity."""
    out = OrderedDict()
    for k, sh in shapes(cfg).items():
        if k.startswith("bn"):
            out[k] = ((1.0 if k.endswith("weight") else 0.0) + 0.2 * rng.randn(*sh)).astype(np.float32)
        else:
            fan_in = shapes(cfg)[k.rsplit(".", 1)[0] + ".weight"][1]
            out[k] = rng.uniform(-1.0, 1.0, size=sh).astype(np.float32) / np.float32(np.sqrt(fan_in))
    return out


def fresh_block(cfg):
    S, H, W = cfg["S"], cfg["H"], cfg["W"]
    z, o = (lambda n: np.zeros(n, np.float32)), (lambda n: np.ones(n, np.float32))
    return OrderedDict([("rms_obs.mean", z(S)), ("rms_obs.var", z(S)), ("rms_obs.count", np.float32(1e-4)), ("rms_ri.mean", z(1)), ("rms_ri.var", z(1)),
                        ("rms_ri.count", np.float32(1e-4)), ("rff.rewems", z(W)), ("bn1.running_mean", z(H)), ("bn1.running_var", o(H)),
                        ("bn2.running_mean", z(FEATURE)), ("bn2.running_var", o(FEATURE)), ("bn1_next.running_mean", z(H)), ("bn1_next.running_var", o(H))])


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
    for k in ("bn1", "bn2", "bn1_next"):
        n = b[k + ".running_mean"].size
        b[k + ".running_mean"] = (0.1 * rng.randn(n)).astype(np.float32)
        b[k + ".running_var"] = (0.5 + rng.rand(n)).astype(np.float32)
    return b


# ---------------------------------------------------------------------------------- running moments and the filter
def moments_merge(mean, var, count, x, dtype=torch.float64):
    """utils.py:26-52: (mean, var, count) after update(x), x [n, ...]."""
    mean, var, count, x = _t(mean, dtype), _t(var, dtype), _t(count, dtype), _t(x, dtype)
    n = x.shape[0]
    b_mean, b_var = x.mean(0), x.std(0) ** 2
    delta, tot = b_mean - mean, count + n
    new_mean = mean + delta * n / tot
    m2 = var * count + b_var * n + delta ** 2 * count * n / (count + n)
    return new_mean, m2 / (count + n), n + count


def filter_states(rewems, r_wt, gamma, dtype=torch.float64):
    """[T, W]: the filter's state after each step of r_wt [W, T] (rewems <- rewems * gamma + r_t)."""
    rew, r = _t(rewems, dtype), _t(r_wt, dtype)
    out = []
    for t in range(r.shape[1]):
        rew = rew * gamma + r[:, t]
        out.append(rew)
    return torch.stack(out)


def aliased_stack(rewems, r_wt, gamma, dtype=torch.float64):
    """What torch.stack([rff.update(r_t) ...]) holds in the reference: T references to ONE Parameter, i.e. T copies of the final state."""
    st = filter_states(rewems, r_wt, gamma, dtype)
    return st[-1:].expand(st.shape[0], -1).contiguous()


# ---------------------------------------------------------------------------------- the network
def _params(weights, dtype, grad):
    return OrderedDict((k, _t(v, dtype).clone().requires_grad_(grad)) for k, v in weights.items())


def normalize_obs(x, blk, dtype):
    return torch.clip((x - _t(blk["rms_obs.mean"], dtype)) / (torch.sqrt(_t(blk["rms_obs.var"], dtype)) + 1e-7), min=-5.0, max=5.0)


def forward(cfg, P, blk, s, a, s2, dtype=torch.float64):
    """icm.py:196-218 without ri_update and the normalisation of r_i.  P: name -> tensor of `dtype`; blk: the block (numpy); the batch norms'
    running statistics are advanced in the returned copy `run`.  -> dict(l_f, l_i, r_raw [b], x_forward, phi, phi_next, z1, z1n, z2: the inputs of bn1, bn1_next, bn2, run)."""
    s, s2, a = _t(s, dtype), _t(s2, dtype), _t(a, dtype).reshape(s.shape[0], -1)
    if cfg["obs_norm"]:
        s, s2 = normalize_obs(s, blk, dtype), normalize_obs(s2, blk, dtype)
    run = {k: _t(blk[k], dtype).clone() for k in BLOCK_KEYS if k.startswith("bn")}
    lin = lambda name, x: F.linear(x, P[name + ".weight"], P[name + ".bias"])
    bn = lambda name, x: F.batch_norm(x, run[name + ".running_mean"], run[name + ".running_var"], P[name + ".weight"], P[name + ".bias"], True, 0.1, 1e-5)
    z1, z1n = lin("fc1", s), lin("fc1", s2)
    if cfg["bn"]:
        h = F.elu(bn("bn1", z1))
        z2 = lin("fc2", h)
        phi = F.elu(bn("bn2", z2))
        hn = F.elu(bn("bn1_next", z1n))
    else:
        h = F.elu(z1)
        z2 = lin("fc2", h)
        phi = F.elu(z2)
        hn = F.elu(z1n)
    phin = F.elu(lin("fc2", hn))  # no batch norm after fc2 on s' (icm.py:32)
    xf = lin("forward_fc2", torch.cat((F.relu(lin("forward_fc1", torch.cat((phi, a), 1))), a), 1))
    l_f = F.mse_loss(xf, phin.detach())
    xi = lin("inverse_fc2", F.relu(lin("inverse_fc1", torch.cat((phi, phin), 1))))
    l_i = F.mse_loss(xi, a) if cfg["cont"] else F.cross_entropy(xi, a.reshape(-1).long())
    r_raw = (cfg["eta"] * 0.5) * torch.sum(torch.abs(xf - phin), 1)
    return dict(l_f=l_f, l_i=l_i, r_raw=r_raw, x_forward=xf, phi=phi, phi_next=phin, z1=z1, z1n=z1n, z2=z2, run=run)


def reward_pass(cfg, weights, blk, s, a, s2, reward, ext=1.0, intr=1.0, dtype=torch.float64):
    """icm_ppo.py:98-102.  -> dict(r_raw, stack [T, W] as the reference builds it, true_stack, r_i, reward, r_i_mean, block: the block after)."""
    with torch.no_grad():
        blk = OrderedDict((k, np.asarray(v).copy()) for k, v in blk.items())
        nb = OrderedDict((k, _t(v, dtype)) for k, v in blk.items())
        nb["rms_obs.mean"], nb["rms_obs.var"], nb["rms_obs.count"] = moments_merge(blk["rms_obs.mean"], blk["rms_obs.var"], blk["rms_obs.count"], s2, dtype)
        out = forward(cfg, _params(weights, dtype, False), nb, s, a, s2, dtype)
        W = cfg["W"]
        r_wt = out["r_raw"].reshape(W, -1)
        true_stack = filter_states(blk["rff.rewems"], r_wt, cfg["gamma"], dtype)
        stack = aliased_stack(blk["rff.rewems"], r_wt, cfg["gamma"], dtype)
        nb["rff.rewems"] = stack[-1]
        nb["rms_ri.mean"], nb["rms_ri.var"], nb["rms_ri.count"] = moments_merge(blk["rms_ri.mean"], blk["rms_ri.var"], blk["rms_ri.count"], stack.reshape(-1, 1), dtype)
        r_i = out["r_raw"] / (torch.sqrt(nb["rms_ri.var"]) + 1e-7) if cfg["ri_norm"] else out["r_raw"]
        nb.update(out["run"])
        mixed = ext * _t(reward, dtype).reshape(-1, 1) + intr * r_i.unsqueeze(1)
        return dict(r_raw=out["r_raw"], stack=stack, true_stack=true_stack, r_i=r_i, reward=mixed, r_i_mean=r_i.mean(), block=nb, l_f=out["l_f"], l_i=out["l_i"])


def clip_(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on a dict of gradients, in place; -> the total norm."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).to(next(iter(grads.values())).dtype)
    if max_norm:
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        for g in grads.values():
            g.mul_(coef)
    return total


def update(cfg, weights, blk, s, a, s2, beta=0.2, max_norm=None, dtype=torch.float64):
    """One minibatch (icm_ppo.py:177, 185, 194-198).  -> dict(l_f, l_i, grads {name: raw gradient}, clipped {name: after clip_grad_norm_},
    norm, run: the batch norms' running statistics after the forward, acts: z1 / z2 / phi / phi_next)."""
    P = _params(weights, dtype, True)
    out = forward(cfg, P, blk, s, a, s2, dtype)
    (beta * out["l_f"] + (1 - beta) * out["l_i"]).backward()
    grads = OrderedDict((k, p.grad.detach().clone()) for k, p in P.items())
    clipped = OrderedDict((k, g.clone()) for k, g in grads.items())
    norm = clip_(clipped, max_norm)
    return dict(l_f=out["l_f"].detach(), l_i=out["l_i"].detach(), grads=grads, clipped=clipped, norm=norm, run=out["run"],
                acts={k: out[k].detach() for k in ("z1", "z1n", "z2", "phi", "phi_next", "x_forward")})


# ---------------------------------------------------------------------------------- cases
def rollout(cfg, rows, rng):
    """state, action, next_state, reward of `rows` transitions: observations on different scales per feature, a few beyond the clip."""
    S, A = cfg["S"], cfg["A"]
    scale = (0.5 + 2.0 * rng.rand(S)).astype(np.float32)
    s = (rng.randn(rows, S) * scale).astype(np.float32)
    s2 = (s + 0.3 * rng.randn(rows, S) * scale).astype(np.float32)
    s[rng.rand(rows, S) < 0.02] *= 8.0
    a = np.tanh(rng.randn(rows, A)).astype(np.float32) if cfg["cont"] else rng.randint(0, A, size=(rows, 1)).astype(np.float32)
    return s, a, s2, rng.randn(rows, 1).astype(np.float32)


UPDATE_ROWS = (2, 3, 16, 33, 63, 64, 65, 130)          # the issue's sweep; 16 / 17 rows: the batch norm kernels' row lanes (a lane with one row, with two)
UPDATE_ROWS_EDGES = (15, 17, 31, 32)                   # both sides of the 16 row lanes and of the tile engine's 32-row tile
REWARD_WT = ((1, 2), (5, 8), (3, 43), (8, 128))        # (W, T): one worker, T below / above the row lanes, config.icm_ppo.cartpole's rollout
REWARD_WT_EDGES = ((257, 2), (4, 4))                   # more workers than the reward kernel's 256 threads; 16 rows = one per row lane


def cases():
    """(tag, cfg, b) of the update kernel cases: the issue's sweeps of b, S (3: ld % 4 != 0), H (16: one column group of the batch norm
    kernels, 48: three, the last GEMM tile half empty), discrete A (2, 3, 39), continuous A (1, 3, 19), batch norm on and off -- each
    dimension swept with the others at a base shape -- plus both sides of the dispatch boundaries named above."""
    out = []
    base = dict(S=4, A=2, H=16, cont=False)
    for b in UPDATE_ROWS + UPDATE_ROWS_EDGES:
        out.append((f"b{b}", config(**base), b))
    for S in (3, 17):
        out.append((f"S{S}", config(**{**base, "S": S}), 33))
    out.append(("H48", config(**{**base, "H": 48}), 33))
    for A in (3, 39):
        out.append((f"A{A}", config(**{**base, "A": A}), 16))
    for A in (1, 3, 19):
        out.append((f"cont_A{A}", config(**{**base, "A": A, "cont": True}), 33))
    out.append(("plain_b1", config(**base, bn=False, obs_norm=False, ri_norm=False), 1))
    out.append(("plain_b33", config(**base, bn=False, obs_norm=False, ri_norm=False), 33))
    out.append(("plain_cont", config(**{**base, "A": 3, "cont": True}, bn=False), 16))
    return out


def reward_cases():
    out = []
    for W, T in REWARD_WT + REWARD_WT_EDGES:
        out.append((f"W{W}_T{T}", config(4, 2, 16, False, W=W), W * T))
    out.append(("cont_W5_T8", config(5, 3, 48, True, W=5), 40))
    out.append(("S3_W3_T43", config(3, 3, 16, False, W=3), 129))
    out.append(("plain_W5_T8", config(4, 2, 16, False, W=5, bn=False, obs_norm=False, ri_norm=False), 40))
    return out


def case_inputs(tag, cfg, rows):
    """(weights, block, state, action, next_state, reward) of a case, from a generator seeded by the tag (the same in every process)."""
    import zlib

    rng = np.random.RandomState(zlib.crc32(tag.encode()) % (1 << 31))
    return (random_weights(cfg, rng), random_block(cfg, rng)) + rollout(cfg, rows, rng)


def update_case(tag, cfg, b):
    """An update case: a rollout of b + 7 rows and the index list that picks its b rows.  -> (weights, block, state, action, next_state, idx)"""
    w, blk, s, a, s2, _ = case_inputs(tag, cfg, b + 7)
    idx = np.random.RandomState(b).permutation(b + 7)[:b].astype(np.int64)
    return w, blk, s, a, s2, idx


def grad_errors(cfg, ours, exact):
    """{segment: max |ours - exact| relative to the segment's largest exact entry}.  One exception: under batch norm fc1.bias sits in front
    of bn1 AND bn1_next, so its exact gradient is zero (1e-17 in float64) and has no scale of its own; what any float32 run leaves there is the
    rounding of sum_r d(z1)[r, c], which is measured against the largest entry of fc1.weight's gradient, the sum of the same terms times x."""
    out = {}
    for k, e in exact.items():
        e = np.asarray(e.detach().cpu() if torch.is_tensor(e) else e, dtype=np.float64)
        o = np.asarray(ours[k].detach().cpu() if torch.is_tensor(ours[k]) else ours[k], dtype=np.float64).reshape(e.shape)
        ref = exact["fc1.weight"] if (k == "fc1.bias" and cfg["bn"]) else e
        ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, dtype=np.float64)
        out[k] = float(np.abs(o - e).max()) / (float(np.abs(ref).max()) + 1e-30)
    return out


def rel(ours, exact):
    """max |ours - exact| relative to max |exact|."""
    exact = np.asarray(exact.detach().cpu() if torch.is_tensor(exact) else exact, dtype=np.float64)
    ours = np.asarray(ours.detach().cpu() if torch.is_tensor(ours) else ours, dtype=np.float64).reshape(exact.shape)
    return float(np.abs(ours - exact).max()) / (float(np.abs(exact).max()) + 1e-30)


# ---------------------------------------------------------------------------------- fixtures of tools/gen_golden_icm.py
FIXTURES = ("icm_discrete", "icm_continuous", "icm_plain", "icm_cartpole")
CURVE_CONFIG = dict(workers=8, n_step=128, iterations=40, seeds=(1, 2, 3), run_step=100000,
                    agent=dict(state_size=4, action_size=2, hidden_size=512, network="discrete_policy_value", head="mlp", optim_config={"name": "adam", "lr": 2.5e-4},
                               gamma=0.99, batch_size=32, n_step=128, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, clip_grad_norm=1.0,
                               use_standardization=False, lr_decay=True, icm_network="icm_mlp", beta=0.2, lamb=1.0, eta=0.1, extrinsic_coeff=1.0,
                               intrinsic_coeff=1.0))  # config/icm_ppo/cartpole.py


def curve_gain(curve):
    """Mean of the last five iterations over the first iteration."""
    return float(np.mean(curve[-5:]) / curve[0])


def icm_recipe(named_shapes, seed):
    """Recipe weights of the module's trainable tensors (oracle.synth's streams, keyed by "icm." + name): linear layers as synth draws them, batch
    norm weights 1 + a draw in +-0.1, biases a draw in +-0.1."""
    from oracle import synth

    out = OrderedDict()
    for k, sh in named_shapes.items():
        v = synth.recipe_tensor("icm." + k, tuple(sh), seed)
        out[k] = np.ascontiguousarray(v + (1.0 if (k.startswith("bn") and k.endswith("weight")) else 0.0), dtype=np.float32)
    return out


class Fixture:
    """One fixture file: hyper-parameters, the rollouts, the starting state_dicts of both networks (stored, or regenerated from the recipe and
    checked against the stored sample) and per learn `l<k>/` what the reference computed."""

    def __init__(self, z):
        from oracle import synth

        self.z = z
        g = lambda k: z[f"hyper/{k}"].item()
        self.S, self.A, self.H, self.W, self.T, self.B = (int(g(k)) for k in ("S", "A", "H", "W", "T", "B"))
        self.M, self.cont, self.limit, self.recipe, self.learns = self.W * self.T, bool(int(g("continuous"))), int(g("thin_limit")), bool(int(g("recipe"))), int(g("learns"))
        self.lr, self.on, self.n_epoch = float(g("lr")), bool(int(g("switches"))), int(g("n_epoch"))
        self.cfg = config(self.S, self.A, self.H, self.cont, W=self.W, gamma=float(g("gamma")), eta=float(g("eta")), obs_norm=self.on, ri_norm=self.on, bn=self.on)
        names = [k[len("sd0/"):] for k in z.files if k.startswith("sd0/")]
        inames = [k[len("icm0/"):] for k in z.files if k.startswith("icm0/")]
        if self.recipe:
            sd = synth.ppo_recipe(OrderedDict((k, tuple(int(s) for s in z[f"shape/{k}"])) for k in names), int(g("recipe_seed")))
            tr = icm_recipe(OrderedDict((k, tuple(int(s) for s in z[f"shape/icm.{k}"])) for k in inames if k in shapes(self.cfg)), int(g("recipe_seed")))
            for k in names:
                assert np.array_equal(self.thin(sd[k]), z[f"sd0/{k}"]), k
            for k in tr:
                assert np.array_equal(self.thin(tr[k]), z[f"icm0/{k}"]), k
            self.sd0 = OrderedDict((k, sd[k]) for k in names)
            self.icm0 = OrderedDict((k, tr[k] if k in tr else z[f"icm0/{k}"]) for k in inames)
        else:
            self.sd0 = OrderedDict((k, z[f"sd0/{k}"]) for k in names)
            self.icm0 = OrderedDict((k, z[f"icm0/{k}"]) for k in inames)

    def thin(self, a):
        from oracle import synth

        a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
        return synth.thin(a, self.limit) if self.limit else a

    def n_minibatch(self):
        return self.n_epoch * ((self.M + self.B - 1) // self.B)

    def rollout(self, k):
        """The transitions of learn k as the list of dicts process() takes."""
        from oracle import synth

        z, p = self.z, f"l{k}/in_"
        if p + "state" in z.files:
            return [{key: z[p + key][i : i + 1] for key in ("state", "action", "reward", "next_state", "done")} for i in range(self.M)]
        trs = synth.ppo_rollout(np.random.RandomState(int(z[f"l{k}/rollout_seed"])), self.M, self.S, self.A, self.cont, clamp_every=0)
        for key in ("state", "reward", "action"):
            got = synth.row_checksum(np.concatenate([t[key] for t in trs], 0).astype(np.float32))[:: max(1, self.M // 64)]
            assert np.array_equal(got, z[f"{p}{key}_check"]), key
        return trs

    def cols(self, k):
        trs = self.rollout(k)
        return {key: np.concatenate([t[key] for t in trs], 0).astype(np.float32) for key in ("state", "action", "next_state", "reward", "done")}

    def sub(self, prefix):
        return OrderedDict((key[len(prefix):], self.z[key]) for key in self.z.files if key.startswith(prefix))

    def agent_kwargs(self):
        g = lambda k: self.z[f"hyper/{k}"].item()
        return dict(state_size=self.S, action_size=self.A, hidden_size=self.H, network="continuous_policy_value" if self.cont else "discrete_policy_value", head="mlp",
                    optim_config={"name": "adam", "lr": self.lr}, gamma=float(g("gamma")), batch_size=self.B, n_step=self.T, n_epoch=self.n_epoch, _lambda=float(g("lambda")),
                    epsilon_clip=float(g("epsilon_clip")), vf_coef=float(g("vf_coef")), ent_coef=float(g("ent_coef")), clip_grad_norm=float(g("clip_grad_norm")),
                    use_standardization=bool(int(g("use_standardization"))), run_step=100000, num_workers=self.W, lr_decay=False, icm_network="icm_mlp",
                    beta=float(g("beta")), lamb=1.0, eta=float(g("eta")), extrinsic_coeff=1.0, intrinsic_coeff=1.0, obs_normalize=self.on, ri_normalize=self.on,
                    batch_norm=self.on)


def load_fixture(name):
    import os

    return Fixture(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False))


def weight_caps(fx, ours, ref, sizes):
    """(fraction of entries further than 2e-5 from the reference's, worst difference / lr) over the tensors of `ours` (full arrays) against
    the fixture's records `ref` (thinned beyond fx.limit entries).  A thinned tensor's sample stands for the whole tensor: its count of far
    entries is scaled by full size / sample size, so a small tensor kept whole does not outweigh the big ones it sits beside."""
    tot = bad = worst = 0.0
    for k, v in ours.items():
        dd = np.abs(fx.thin(np.asarray(v, dtype=np.float64)).reshape(-1) - np.asarray(ref[k], dtype=np.float64).reshape(-1))
        n = float(sizes[k])
        tot, bad, worst = tot + n, bad + float((dd > 2e-5).sum()) * n / dd.size, max(worst, float(dd.max()) / fx.lr)
    return bad / tot, worst
