"""The float64 truth of tests/sacd_truth.py against the reference's own learn() (the fixtures of tools/gen_golden_sac_discrete.py) and against torch's
autograd on the tie and near-clamp rows, and the conditions the GPU cases rely on: each case's recorded float32 gap, no accidental tie, the clamp's margins."""
import numpy as np
import pytest
import torch

import sacd_truth as D
from tests.util import load

TOL = 1e-5


def _close(got, want, what):
    np.testing.assert_allclose(np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1), rtol=TOL, atol=TOL, err_msg=what)


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_matches_the_reference_records(name):
    z = load(name)
    for r in (f"r{i}" for i in range(int(z["hyper/records"]))):
        g = lambda k: z[f"{r}/learn/{k}"]
        alpha, la = float(z[f"{r}/alpha0/alpha"]), float(z[f"{r}/alpha0/log_alpha"])
        cr = D.critic_loss(g("logits_next"), g("qt1_next"), g("qt2_next"), g("q1_all"), g("q2_all"), g("action"), g("reward"), g("done"), float(z["hyper/gamma"]), alpha)
        ac = D.actor_loss(g("logits"), g("q1_after"), g("q2_after"), alpha, la, float(z["hyper/target_entropy"]))
        for got, key in ((cr["y"], "target_q"), (cr["next_q"][0], "next_q1"), (cr["next_q"][1], "next_q2"), (cr["H"], "entropy_next"), (cr["grad"][0], "d_q1_all"),
                         (cr["grad"][1], "d_q2_all"), (ac["q"][0], "q1_pi"), (ac["q"][1], "q2_pi"), (ac["grad"], "d_logits"), (ac["actor_loss"], "actor_loss")):
            _close(got, g(key), f"{name} {r} {key}")
        res = dict(critic_loss1=cr["loss"][0], critic_loss2=cr["loss"][1], max_Q=cr["max_Q"], actor_loss=ac["actor_loss"], alpha_loss=ac["alpha_loss"],
                   mean_Q=ac["mean_Q"], alpha=ac["alpha"], entropy=ac["entropy"])
        for k, v in res.items():
            _close(v, z[f"{r}/result/{k}"], f"{name} {r} result {k}")
        if int(z["hyper/use_dynamic_alpha"]):
            a0 = {k: float(z[f"{r}/alpha0/{k}"]) for k in ("exp_avg", "exp_avg_sq", "step")}
            stepped = D.adam_scalar(la, ac["g_log_alpha"], a0["exp_avg"], a0["exp_avg_sq"], a0["step"] + 1, float(z["hyper/alpha_lr"]))
            for got, key in zip(stepped, ("log_alpha", "exp_avg", "exp_avg_sq")):
                np.testing.assert_allclose(got, float(z[f"{r}/alpha1/{key}"]), rtol=TOL, err_msg=f"{name} {r} alpha1 {key}")
        else:
            assert float(z[f"{r}/alpha1/log_alpha"]) == la


@pytest.mark.parametrize("c", [c for c in D.CASES if (c.get("tie") or c.get("near")) and c["B"] <= 129], ids=D.case_id)
def test_truth_gradient_matches_torch_autograd_on_ties_and_near_the_clamp(c):
    """The fixtures hold no tie and no clamped probability: the truth's 0.5 / 0.5 rule and its zeroed derivative under the clamp are pinned to torch.min's
    and Categorical's own backward (float32, as the reference runs them)."""
    x = D.case_inputs(c)
    la = torch.tensor(x["la"], requires_grad=True)
    pi = torch.softmax(la, -1)
    q1, q2 = ((pi * torch.tensor(x[k])).sum(-1) for k in ("q1_pi", "q2_pi"))
    (-(float(np.float32(D.ALPHA)) * torch.distributions.Categorical(probs=pi).entropy() + torch.min(q1, q2))).mean().backward()
    want = D.actor_loss(x["la"], x["q1_pi"], x["q2_pi"], float(np.float32(D.ALPHA)), D.LOG_ALPHA, 0.0)["grad"]
    assert not c.get("tie") or torch.equal(q1[:1], q2[:1]), "torch sees the tie"
    err = np.abs(la.grad.numpy() - want).max() / np.abs(want).max()  # a wrong tie weight: 0.1 and more; the derivative under the clamp kept: 1e-4
    print(f"{D.case_id(c)}: {err:.3e}")
    assert err <= TOL


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_case_conditions_and_recorded_float32_gap(c):
    x, B = D.case_inputs(c), c["B"]
    want, _, cr, ac = D.case_truth(c)
    gap, where = D.distance(D.case_truth(c, np.float32)[0], want)
    print(f"{D.case_id(c)}: float32 gap {gap:.4e} at {where}, recorded {c['gap']:.4e}")
    assert c["gap"] / 1.02 <= gap <= c["gap"], "the recorded gap is not this case's: recompute it"
    for e, what in ((ac["q"], "actor"), (cr["next_q"], "critic")):  # ties: only where the case makes one, exact there, and from different Q rows
        sep = np.abs(e[0] - e[1]) / np.maximum(np.abs(e[0]), np.abs(e[1]))
        assert np.all(sep[int(bool(c.get("tie"))):] > 1e-5), f"{what}: an accidental near-tie"
        assert not c.get("tie") or (sep[0] == 0.0 and not np.array_equal(x["q1_pi"][0], x["q2_pi"][0]) and not np.array_equal(x["qt1"][0], x["qt2"][0]))
    assert B == 1 or (x["done"][0] == 1 and x["done"][1] == 0), "a terminal and a non-terminal row"
    # the clamp.  Float32 places a log-probability within 1e-5 of float64's: a margin of 1 (a factor e in p) is wide for which side of log eps it falls on.
    # Rows that bind: the last (B >= 2) by 20 and more, at both ends; every row of a "near" case by 1 .. 4 at the low end only.  All else clear of both ends.
    lo, hi = np.log(D.EPS), np.log1p(-D.EPS)
    for k in ("la", "la_next"):
        zs = x[k].astype(np.float64) - x[k].max(1, keepdims=True)
        lp = zs - np.log(np.exp(zs).sum(1, keepdims=True))
        low, binds = lp < lo, np.zeros(B, bool)
        binds[:] = bool(c.get("near"))
        binds[-1] |= B >= 2
        assert np.array_equal(low.sum(1) > 0, binds) and np.all(low[binds].sum(1) == c["A"] - (2 if c.get("near") else 1))
        assert np.all((lp[low] < lo - 1) & (lp[low] > lo - 4)) if c.get("near") else np.all(lp[low] < lo - 20)
        assert np.all(lp[~low] > lo + 2) and np.all((lp[~low] < 1e3 * hi) | (lp[~low] > 1e-6 * hi))
