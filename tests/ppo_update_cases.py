"""Case table and input generator of tests/test_ppo_update_rows_gpu.py (jh_pponet_ppo_update_rows against a float64 evaluation of the same
update, tests/fp64_truth.py: ppo_update_float64).  Imports neither the product nor the oracle: the CPU suite (test_ppo_update_truth_cpu.py) checks
the generator's conditions for every case without a GPU.

A whole-update gradient sums over the rows, so a row that sits on a kink of the loss cannot be masked out of the comparison: the inputs are
built FROM the float64 heads (forward first, then log pi_old, V_old and the return are placed around them) such that, evaluated in float64 on
the fp32 inputs the kernels get,

  * every row's ratio is further than 1e-3 from 1 - eps and 1 + eps, and | |v - v_old| - eps | > 1e-3            (no row excluded)
  * min_prob, the smallest pi(a|s) of the minibatch, is a normal fp32 number (> 1e-30)
  * the regimes that pin the critic's branch have |c1 - c2| > 1e-3 max(c1, c2)
  * between a fifth and four fifths of the rows have the value clamp binding, and likewise the ratio clip under each sign of the advantage
    (minibatches of >= 255 rows; smaller ones: every row binds, so that the branch is pinned)

Critic regimes:
  "c1"    c1 > c2: the unclipped branch carries the gradient (w1 = 1)
  "c2"    c2 > c1 (w1 = 0)
  "own"   value_old = this network's own value (every learn()'s first minibatch): no clamp binds, c1 and c2 are equal or an ulp apart; the branch
          condition is replaced by: both branches' value gradients coincide in float64
  "tail"  the branch is decided by the rows of the LAST loss workgroup (rows 256 (nb - 1) ..): the first nb - 1 workgroups' sums favour one
          branch, the total the other, and every row of the last workgroup has the value clamp binding -- a reduction of the loss partials that
          drops the last one (a partial last wave of jh_mlp_heads_bwd_dh_kernel) then gives those rows the other branch's gradient

ReLU kinks are not handled: the criterion (fp64_truth.vs_exact) carries torch-CPU-fp32's own error, which has the same flips."""
import collections
import zlib

import numpy as np
import torch

import fp64_truth as T

Case = collections.namedtuple("Case", "cont S H A B M regime max_norm")  # M = 0: idx=None (the rows in order), else B of M rows through a permutation

D, C = False, True
# Not a cross product: every boundary of the dispatch inside jh_pponet_ppo_update_rows once with each policy kind.  Nothing of the issue's list is trimmed;
# H = 512 stays at B <= 2049 (the float64 evaluation on the CPU).
CASES = [
    # ---- B at every boundary, from both sides (1024: fused loss kernel | one-pass; gemm16 | tile engine.  2048: fused forward | tiled.  16384: consumer | ticket)
    Case(D, 4, 64, 2, 1, 50, "own", 0.5), Case(C, 11, 64, 3, 1, 50, "c1", 0.5),
    Case(D, 4, 64, 2, 255, 600, "c2", 0.5), Case(C, 3, 64, 1, 255, 600, "c1", 0.5),
    Case(D, 8, 64, 7, 1023, 0, "c1", 0.5), Case(C, 11, 64, 3, 1023, 1500, "c2", 0.5),
    Case(D, 4, 64, 2, 1024, 1500, "c2", 0.5), Case(C, 11, 64, 3, 1024, 1500, "own", 0.5),
    Case(D, 4, 64, 2, 1025, 1500, "c1", 1e4), Case(C, 11, 64, 3, 1025, 1500, "c2", 0.5),
    Case(D, 9, 64, 6, 2047, 2500, "c2", 0.5), Case(C, 16, 64, 3, 2047, 2500, "c1", 0.5),
    Case(D, 4, 64, 2, 2048, 3000, "own", 0.5), Case(C, 11, 64, 3, 2048, 3000, "c1", 1e-4),
    Case(D, 17, 64, 2, 2049, 3000, "c1", 0.5), Case(C, 27, 64, 8, 2049, 3000, "c2", 0.5),  # (S > 16: scalar layer 1, dW1 by row gather + GEMM; 17 outputs: value head in the third launch)
    Case(D, 4, 64, 2, 16384, 17000, "c1", 0.5), Case(C, 11, 64, 3, 16384, 0, "c2", 0.5),
    Case(D, 4, 64, 2, 16385, 17000, "c2", 0.0), Case(C, 11, 64, 3, 16385, 17000, "c1", 0.5),
    Case(D, 4, 64, 2, 20011, 21000, "own", 0.5), Case(C, 11, 64, 3, 20011, 21000, "c2", 1e4),
    # ---- a partial last wave in jh_mlp_heads_bwd_dh_kernel (B H / 4 % 64 != 0); (H 16, B 1041) and (H 64, B 4101): more loss partials than live lanes
    Case(D, 4, 16, 2, 1041, 1500, "tail", 0.5), Case(C, 11, 16, 3, 1041, 1500, "tail", 0.5),
    Case(D, 3, 32, 6, 1027, 1500, "tail", 0.5), Case(C, 8, 32, 3, 1027, 1500, "tail", 0.5),
    Case(D, 4, 64, 2, 1030, 1500, "tail", 0.5), Case(C, 11, 64, 3, 1030, 1500, "tail", 0.0),
    Case(D, 4, 128, 2, 1025, 1500, "tail", 0.5), Case(C, 9, 128, 4, 1025, 1500, "tail", 0.5),  # (9 outputs: value head alone in the second launch)
    Case(D, 4, 64, 2, 4101, 5000, "tail", 0.5), Case(C, 11, 64, 3, 4101, 5000, "tail", 0.5),
    # ---- hidden widths: 48 is not jh_pmb_eligible; 512 the baseline width
    Case(D, 4, 48, 2, 300, 600, "c2", 1e-4), Case(C, 11, 48, 3, 1500, 2000, "c1", 0.5),
    Case(D, 4, 512, 2, 1025, 1500, "c2", 0.5), Case(C, 11, 512, 3, 2049, 3000, "c1", 0.5), Case(C, 17, 512, 6, 1023, 1500, "own", 0.5),
    # ---- head outputs 8 / 13 / 17 with the value head in the first / second / third launch, above and below 1024 rows
    Case(D, 8, 64, 7, 1500, 2000, "c1", 0.5), Case(C, 17, 64, 6, 1100, 1500, "c1", 0.5), Case(D, 6, 32, 12, 2100, 2500, "c2", 0.5),
    Case(D, 5, 64, 16, 300, 600, "c1", 0.5),
    # ---- a hidden row narrower than the packed head gradient (gld 20 > H 16, gld 36 > H 32) above 1024 rows
    Case(C, 27, 16, 8, 1100, 1500, "c2", 0.5), Case(C, 9, 32, 16, 1041, 1500, "tail", 0.5),
]


def case_id(c):
    return f"{'cont' if c.cont else 'disc'}-S{c.S}-H{c.H}-A{c.A}-B{c.B}-{'M%d' % c.M if c.M else 'noidx'}-{c.regime}-clip{c.max_norm:g}"


IDS = [case_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)

ENT = 0.01
LR = 1e-3


def hyper(c):
    """-> eps_clip, vf_coef, ent_coef of the case"""
    return (0.2 if c.cont else 0.1), (0.5 if c.H in (48, 128) else 1.0), ENT


def module_of(c):
    """The case's network (tests/mirror) in float64 with fp32-representable weights.  Deterministic per case."""
    from mirror.networks import Network

    torch.manual_seed(zlib.crc32(case_id(c).encode()))
    m = Network("continuous_policy_value" if c.cont else "discrete_policy_value", c.S, c.A, D_hidden=c.H).double()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return T.round_to_fp32_(m)


def _two_sided(n, lo0, lo1, hi0, hi1, p_hi):
    """n draws: with probability p_hi from [hi0, hi1], else from [lo0, lo1].  -> (values float64, picked-hi mask)"""
    hi = torch.rand(n) < p_hi
    u = torch.rand(n, dtype=torch.float64)
    return torch.where(hi, hi0 + (hi1 - hi0) * u, lo0 + (lo1 - lo0) * u), hi


def make(c):
    """-> dict: module (float64), x [M, S], idx (int64 [B] | None), action, adv, ret, value_old, logp_old ([M, .] float32, the layout
    PPONet.ppo_update_rows takes), eps, vf, ent.  Rows outside idx hold unrelated values (a wrong gather shows)."""
    module = module_of(c)
    eps, vf, ent = hyper(c)
    B, M, A = c.B, (c.M or c.B), c.A
    x = torch.randn(M, c.S)
    idx = torch.randperm(M)[:B].contiguous() if c.M else None
    sel = idx if idx is not None else torch.arange(B)
    with torch.no_grad():
        heads = module.raw(x[sel].double())
    v = heads[-1].reshape(-1)
    # ---- policy side: log pi_old = log pi - log(wanted ratio), the wanted ratio inside the clip range or well outside on either side
    if c.cont:
        # actions as a rollout has them: drawn from (a policy near) this one, so that no log pi falls out of fp32's range -- min_prob is an fp32 statistic
        dist = torch.distributions.Normal(torch.clamp(heads[0], -5.0, 5.0), torch.tanh(heads[1]).exp())
        action = torch.tanh((dist.loc + dist.scale * torch.randn(B, A, dtype=torch.float64).clamp(-2.5, 2.5)).clamp(-3.0, 3.0)).float()
        logp = dist.log_prob(torch.atanh(torch.clamp(action, -1 + 1e-7, 1 - 1e-7).double()))
    else:
        action = torch.randint(0, A, (B, 1)).float()
        logp = torch.log_softmax(heads[0], dim=-1).gather(1, action.long())
    ncol = logp.shape[1]
    out, is_out = _two_sided(B, 1.0 - 0.5 * eps, 1.0 + 0.5 * eps, 1.5 * eps, 3.0 * eps, 0.6 if B >= 16 else 1.0)
    side = torch.where(torch.rand(B) < 0.5, -1.0, 1.0).double()
    want = torch.where(is_out, 1.0 + side * out, out)  # inside: [1 - eps/2, 1 + eps/2]; outside: 1 +- [1.5 eps, 3 eps]
    logp_old = (logp - (want.log() / ncol).unsqueeze(1)).float()
    adv = torch.randn(B, 1)
    # ---- critic side: |v - v_old| in [0, eps / 2] or [1.5 eps, 3 eps]; the return a unit away from v on the side that favours the wanted branch
    if c.regime == "own":
        value_old = v.float()
        ret = (v + torch.randn(B, dtype=torch.float64)).float()
    else:
        d, binds = _two_sided(B, 0.0, 0.5 * eps, 1.5 * eps, 3.0 * eps, 0.5 if B >= 16 else 1.0)
        s = torch.where(torch.rand(B) < 0.5, -1.0, 1.0).double()  # sign of v - v_old
        n_last = B - 256 * ((B + 255) // 256 - 1)
        last = torch.arange(B) >= B - n_last
        if c.regime == "tail":
            d = torch.where(last, eps + (0.5 + 1.5 * torch.rand(B, dtype=torch.float64)) * eps, d)
            binds = binds | last
        value_old = (v - s * d).float()
        # v_clip lies between v_old and v: a return on v_old's side of v makes |v - ret| the larger error (c1 > c2), one beyond v the smaller
        fav1 = {"c1": torch.ones(B, dtype=torch.bool), "c2": torch.zeros(B, dtype=torch.bool), "tail": torch.rand(B) < 0.6}[c.regime]
        off = 1.0 + 0.1 * torch.randn(B, dtype=torch.float64).clamp(-3, 3)
        ret = v + torch.where(fav1, -s, s) * off
        if c.regime == "tail":
            assert B > 256, "the tail regime needs more than one loss workgroup"
            dvo = v - value_old.double()
            e1 = (v - ret) ** 2
            e2 = (value_old.double() + dvo.clamp(-eps, eps) - ret) ** 2
            dfirst = float((e1 - e2)[~last].sum())
            delta = (dvo.abs() - eps)[last]
            k = max(1.0, (2.0 * abs(dfirst) + float((delta ** 2).sum())) / (2.0 * float(delta.sum())))
            sgn = torch.sign(dvo)
            ret = torch.where(last, v + (sgn if dfirst > 0 else -sgn) * k, ret)
        ret = ret.float()

    def full(rows, junk):
        if idx is None:
            return rows.contiguous()
        junk[idx] = rows
        return junk.contiguous()

    return {
        "module": module, "x": x, "idx": idx, "eps": eps, "vf": vf, "ent": ent,
        "action": full(action, torch.tanh(torch.randn(M, A)) if c.cont else torch.randint(0, A, (M, 1)).float()),
        "adv": full(adv, 3.0 * torch.randn(M, 1)), "ret": full(ret.reshape(-1, 1), 3.0 * torch.randn(M, 1)),
        "value_old": full(value_old.reshape(-1, 1), 3.0 * torch.randn(M, 1)), "logp_old": full(logp_old, -torch.rand(M, ncol) - 0.3),
    }


def gathered(inp):
    """The minibatch's rows of every per-row input, in minibatch order."""
    sel = inp["idx"] if inp["idx"] is not None else slice(None)
    return {k: inp[k][sel] for k in ("x", "action", "adv", "ret", "value_old", "logp_old")}


def truth(c, inp, module=None):
    """ppo_update_float64 on the case's inputs with `module` (default: the float64 one)."""
    r = gathered(inp)
    return T.ppo_update_float64(module if module is not None else inp["module"], c.cont, r["x"], r["action"], r["adv"], r["ret"], r["value_old"], r["logp_old"],
                                inp["eps"], inp["vf"], inp["ent"])


def check_conditions(c, inp, exact):
    """The conditions of the module docstring on the float64 evaluation `exact` = truth(c, inp): asserted, nothing excluded.  -> the shares (for the record)."""
    eps = inp["eps"]
    _, stats, grads, rows = exact
    ratio, dv = rows["ratio"], rows["dv"]
    B = c.B
    assert ratio.numel() == B and all(bool(torch.isfinite(g).all()) for g in grads.values())
    kink_r = float(torch.minimum((ratio - (1 - eps)).abs(), (ratio - (1 + eps)).abs()).min())
    kink_v = float((dv.abs() - eps).abs().min())
    assert kink_r > 1e-3, f"a ratio {kink_r:.2e} from the clip bound"
    assert kink_v > 1e-3, f"a |v - v_old| {kink_v:.2e} from eps"
    assert stats["min_prob"] > 1e-30, stats["min_prob"]
    c1, c2 = stats["c1"], stats["c2"]
    v_binds = dv.abs() > eps
    r_binds = (ratio - 1).abs() > eps
    adv = gathered(inp)["adv"].reshape(-1)
    out = {"kink_ratio": kink_r, "kink_value": kink_v, "min_prob": stats["min_prob"], "c1": c1, "c2": c2, "value_clamp_share": float(v_binds.double().mean())}
    if c.regime == "own":
        assert not bool(v_binds.any())
        diff = float((rows["g_c1"] - rows["g_c2"]).abs().max())
        assert diff <= 1e-12 * float(rows["g_c1"].abs().max()), f"the two branches' value gradients differ by {diff:.2e}"
    else:
        assert abs(c1 - c2) > 1e-3 * max(c1, c2), (c1, c2)
        assert {"c1": c1 > c2, "c2": c2 > c1, "tail": True}[c.regime], (c1, c2)
        if B >= 255:
            assert 0.2 <= out["value_clamp_share"] <= 0.8, out
        else:
            assert bool(v_binds.all())
    if B >= 255:
        for name, m in (("adv>0", adv > 0), ("adv<0", adv < 0)):
            share = float(r_binds[m].double().mean())
            out[f"ratio_clip_share_{name}"] = share
            assert 0.2 <= share <= 0.8, (name, share)
            # ... and both sides of the range under each sign: one side's gradient is cut, the other's passes
            assert bool((ratio[m] > 1 + eps).any()) and bool((ratio[m] < 1 - eps).any())
    norm = float(torch.sqrt(sum((g ** 2).sum() for g in grads.values())))
    out["grad_norm"] = norm
    if c.max_norm > 0 and c.max_norm != 0.5:  # the clip far from its threshold on either side (0.5, the agent's default, falls where it falls)
        assert norm > 10 * c.max_norm or norm < 0.1 * c.max_norm, (norm, c.max_norm)
    if c.regime == "tail":
        r = gathered(inp)
        with torch.no_grad():
            v = exact[0][-1].reshape(-1)
            vo, ret = r["value_old"].double().reshape(-1), r["ret"].double().reshape(-1)
            e1, e2 = (v - ret) ** 2, (vo + (v - vo).clamp(-eps, eps) - ret) ** 2
        n_first = 256 * ((B + 255) // 256 - 1)
        f1, f2 = float(e1[:n_first].sum()), float(e2[:n_first].sum())
        assert abs(f1 - f2) > 1e-3 * max(f1, f2) and (f1 > f2) != (c1 > c2), ("the last loss workgroup does not decide the branch", f1, f2, c1, c2)
        assert bool(v_binds[n_first:].all())
        out["first_workgroups"] = (f1, f2)
    return out
