"""CPU-side checks of continuous MPO's kernels: the C ABI, the binding table and jorldy_amd.ops carry jh_mpo_sample and jh_mpo_loss_continuous,
the float64 numpy statement in tests/mpo_cont_truth.py agrees with the reference's own formulas evaluated by torch autograd in float64 (losses,
head gradients, all three multipliers' gradients), and the case builders have the properties the GPU tests rely on -- among them that no case
sits near the c = 1 clip or the +-5 clamp, where a last-bit difference would change the branch; the agent's eligibility, decided before any
GPU use; and the float64 statement against every tapped tensor of the reference's own learn() in the fixtures of
tools/gen_golden_mpo_continuous.py, at half the tolerances the GPU tests give the kernels."""
import os
import re

import numpy as np
import pytest
import torch

import mpo_cont_truth as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("jh_mpo_sample", "jh_mpo_loss_continuous")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_binding_table_and_ops_carry_the_new_entries(lib):
    from jorldy_amd import _lib, ops

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "mpo.py:199-309" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert callable(ops.mpo_sample) and callable(ops.mpo_loss_continuous)
    assert (ops.MPO_MAX_ROWS, ops.MPO_MAX_SAMPLED, ops.MPO_MAX_CONT_ACTIONS) == (D.MAX_ROWS, D.MAX_SAMPLED, D.MAX_ACTIONS)
    assert D.STATS == ops.MPO_STATS
    # the continuous kernel steps the multipliers with the one shared copy
    s = open(os.path.join(ROOT, "jorldy_amd", "csrc", "jh_mpo.hip")).read()
    assert s.count("multiplier_step(a.blk, 2,") == 1 and "float multiplier_step(" not in s


def test_the_caps_admit_every_continuous_config_of_the_reference_and_refuse_the_class_defaults():
    ok = lambda B, T, N, A: B * T <= D.MAX_ROWS and N * B * T <= D.MAX_SAMPLED and 1 <= N and 1 <= A <= D.MAX_ACTIONS
    assert ok(64, 4, 30, 1)          # config.mpo.pendulum: 7680 sampled rows
    assert ok(32, 1, 30, 3)          # config.mpo.hopper_mlagent / drone_delivery_mlagent (1step_TD): 960
    assert not ok(64, 8, 30, 2)      # the class defaults: 15360
    assert D.MAX_ACTIONS >= 8


@pytest.mark.parametrize("R,T,N,A", D.LOSS_CASES, ids=[f"R{r}-T{t}-N{n}-A{a}" for r, t, n, a in D.LOSS_CASES])
def test_numpy_truth_equals_the_reference_formulas_in_float64(R, T, N, A):
    """The numpy statement (row maximum, sum of logs) against the reference's own lines under autograd in float64: equal to 1e-12 where the
    reference's formulas are finite (eta = 0.7)."""
    c = D.case(R, T, N, A)
    for retrace in ((True, False) if T > 1 else (True,)):
        t, t64 = D.case_truth(c, retrace), D.case_truth(c, retrace, torch.float64)
        for key in ("actor", "critic", "eta_loss", "alpha_loss"):
            assert abs(t64[key] - t[key]) <= 1e-12 * (abs(t[key]) + 1.0), key
        for key in ("qret", "c"):
            assert np.abs(t64[key] - t[key]).max() <= 1e-12 * (np.abs(t[key]).max() + 1.0), key
        for key in ("head", "q"):
            assert np.abs(t64["grads"][key] - t["grads"][key]).max() <= 1e-12 * np.abs(t["grads"][key]).max() + 1e-18, key
        for j in range(3):
            assert abs(t64["mult_grads"][j] - t["mult_grads"][j]) <= 1e-11 * t["mult_scale"][j], D.NAMES[j]


def test_sample_truth_equals_torch_in_float64():
    for R, _, N, A in D.SAMPLE_CASES:
        c = D.sample_case(R, N, A)
        t, t64 = D.sample(**c), D.sample_torch(**c, dtype=torch.float64)
        for k in ("zn", "zt_add", "a_next", "a_add"):
            assert t[k].shape == (N, R, A) and np.abs(t[k] - t64[k]).max() <= 1e-13 * (np.abs(t[k]).max() + 1.0), k
        assert (np.abs(c["head_next"][:, :A]) > 5).any() and (np.abs(c["head_old"][:, :A]) > 5).any(), "the clamp is exercised"


def test_case_builders_have_the_properties_the_gpu_tests_rely_on():
    assert [(r, n * r) for r, _, n, _ in D.LOSS_CASES][-2] == (D.MAX_ROWS, D.MAX_SAMPLED), "both caps at once"
    assert D.LOSS_CASES[-1][3] == D.MAX_ACTIONS
    for variant in ("plain", "hot", "floor", "alldone"):
        for R, T, N, A in D.LOSS_CASES:
            c = D.case(R, T, N, A, variant)
            t = D.case_truth(c)
            clip, clamp = D.distance_from_the_switches(t)
            assert clip > 1e-4 and clamp > 1e-4, (variant, R, T, N, A, clip, clamp)
            assert (np.abs(t["mu_raw"]) > 5).any(), "a clamped raw mu: zero gradient there"
            assert not t["grads"]["head"][:, :A][np.abs(t["mu_raw"]) > 5].any() and np.isfinite(t["grads"]["head"]).all()
            if R >= 3:
                assert (c["action"] == 1.0).any() and (c["action"] == -1.0).any(), "saturated stored actions"
                assert np.isfinite(t["z"]).all() and np.abs(t["z"]).max() == pytest.approx(np.arctanh(D.ATANH_BOUND))
                assert (t["c"] == 1.0).any() and (t["c"] < 1.0).any(), "prob_b on both sides of the clip"
            if T > 1:
                assert c["done"].reshape(-1, T)[:, : T - 1].any() and c["done"][T - 2] == 1.0
                assert np.array_equal(D.case_truth(c, retrace=False)["qret"], t["qret0"])
                if variant != "alldone":
                    assert not np.array_equal(t["qret0"], t["qret"])
            if N == 1:
                assert not t["At"].any() and (t["w"] == 1.0).all(), "the degenerate E-step"
    c = D.case(64, 4, 30, 3, "alldone")
    t = D.case_truth(c)
    assert c["done"][:4].all() and np.array_equal(t["qret"][:4], c["reward"][:4].astype(np.float64)), "a trajectory whose every step is done keeps its rewards"
    c = D.case(64, 4, 30, 3, "hot")
    t64, t32 = D.case_truth(c), D.case_truth(c, dtype=torch.float32)
    assert float(np.abs(t64["At"]).max()) / 1e-3 > 100.0
    assert np.isfinite(t64["eta_loss"]) and np.isfinite(t64["mult_grads"][0]) and not np.isfinite(t32["eta_loss"]), "float64 around the row maximum holds, float32 exp overflows"
    c = D.case(20, 4, 6, 3, "floor")
    t = D.case_truth(c)
    for j in range(3):
        w, _, _ = D.multiplier_step(c["mult"][j], t["mult_grads"][j], c["m"][j], c["v"][j], D.STEP0, D.LR, c["floors"][j], D.BETAS, D.ADAM_EPS)
        assert w == float(c["floors"][j]), f"the step of {D.NAMES[j]} crosses its floor"


# ---------------------------------------------------------------------------------------------- the agent's eligibility, before any GPU use
def _mpo(**kw):
    from jorldy_amd.core.agent import Agent

    base = dict(state_size=4, action_size=2, actor="continuous_policy", critic="continuous_q_network")
    base.update(kw)
    return Agent("mpo", **base)


@pytest.mark.parametrize("kw", [dict(state_size=3, action_size=1, batch_size=64, n_step=4), dict(state_size=76, action_size=3, batch_size=32, n_step=1, critic_loss_type="1step_TD"),
                                dict(batch_size=1024, n_step=8, num_sample=8, critic_loss_type="1step_TD"), dict(action_size=8, batch_size=8, n_step=4)],
                         ids=["pendulum", "hopper_mlagent", "both_caps", "A_8"])
def test_eligible_continuous_configurations_reach_the_device_check(kw, lib):
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _mpo(**kw)


@pytest.mark.parametrize("kw", [dict(), dict(critic="discrete_q_network"), dict(actor="discrete_policy"), dict(batch_size=8, n_step=4, head="cnn", state_size=(4, 84, 84)),
                                dict(batch_size=8, n_step=4, grad_sync=object()), dict(batch_size=8, n_step=4, num_sample=0), dict(batch_size=8, n_step=4, num_sample=2.5),
                                dict(batch_size=8, n_step=4, optim_config={"name": "rmsprop"}), dict(batch_size=8, n_step=4, action_size=9),
                                dict(batch_size=8, n_step=4, action_size=0), dict(batch_size=64, n_step=4, num_sample=33), dict(batch_size=129, n_step=8, num_sample=1),
                                dict(batch_size=8, n_step=4, hidden_size=30)],
                         ids=["class_defaults_15360", "discrete_critic", "discrete_actor", "cnn", "grad_sync", "num_sample_0", "num_sample_2.5", "rmsprop", "A_9", "A_0",
                              "sampled_8448", "rows_1032", "hidden_30"])
def test_continuous_configurations_outside_the_native_engine_raise_the_sentence(kw):
    with pytest.raises(ValueError, match="MPO runs on libjorldy_hip only") as e:
        _mpo(**kw)
    for word in ("discrete_policy", "discrete_q_network", "continuous_policy", "continuous_q_network", "cnn", "grad_sync", "batch_size \\* n_step <= 1024",
                 "num_sample \\* batch_size \\* n_step <= 8192", "action_size <= 8", "not available for this agent"):
        assert re.search(word, str(e.value)), word


def test_agent_dispatch_keeps_one_registered_class():
    from jorldy_amd.core.agent import agent_dict
    from jorldy_amd.core.agent.mpo import MPO, MPOContinuous

    assert agent_dict["mpo"] is MPO and issubclass(MPOContinuous, MPO)
    assert type(MPO.__new__(MPO)) is MPO and type(MPO.__new__(MPO, 4, 2, actor="continuous_policy")) is MPOContinuous
    for name in ("__init__", "process", "interact_callback", "learning_rate_decay", "save", "load", "_resume_extra_attrs", "_resume_load_extra_attrs", "sync_in", "sync_out", "_run_learn"):
        assert getattr(MPOContinuous, name) is getattr(MPO, name), f"{name} has one copy"


# ---------------------------------------------------------------------------------------------- the fixtures of tools/gen_golden_mpo_continuous.py
def _half(err, tol, what):
    assert err <= 0.5 * tol, f"{what}: {err:.3e} is more than half of the GPU test's tolerance {tol:.3e}"


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a.reshape(b.shape) - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    """Float64 on the reference's tapped inputs against its own float32 run, every learn, at no more than half of the GPU test's tolerance: the
    sampling (z from the stored eps), c, Qret before and after the scan, At, the E-step weights, both KLDs, the four losses, head gradients and dQ,
    the three multipliers' gradients (against the magnitude of their terms), their step (fp64_truth's per-element criterion) and moments."""
    fx = D.Fixture(name)
    assert fx.R == fx.B * fx.T and fx.NS * fx.R <= D.MAX_SAMPLED
    for k in range(fx.learns):
        rec = fx.learn(k)
        t, mult0 = D.fixture_truth(fx, rec)
        for z, mu, std, e in ((rec["zn"], rec["next_mu"], rec["next_std"], rec["eps"][0]), (rec["zt_add"], rec["mut"], rec["stdt"], rec["eps"][1])):
            back = mu.astype(np.float64)[None] + std.astype(np.float64)[None] * e.astype(np.float64)
            _half(float(np.abs(back - z).max()), 1e-5 * float(np.abs(z).max()) + 2e-5, f"l{k} z from the stored eps")
        for key, ref, tol in (("actor", "actor_loss", fx.tol("actor_loss")), ("critic", "critic_loss", 1e-5), ("eta_loss", "eta_loss", fx.tol("eta_loss")),
                              ("alpha_loss", "alpha_loss", fx.tol("alpha_loss"))):
            _half(_rel(rec[ref], t[key]), tol, f"l{k} {ref}")
            assert float(rec[ref]) == float(rec[f"result/{ref}"])
        for key in ("c", "qret0", "qret"):
            _half(_rel(rec[key], t[key]), 1e-5, f"l{k} {key}")
        for key, tk in (("At", "At"), ("w", "w"), ("kld_mu", "kld_mu"), ("kld_sigma", "kld_sigma")):
            _half(float(np.abs(rec[key].astype(np.float64).reshape(t[tk].shape) - t[tk]).max()), fx.tol("At" if key == "At" else "w") * float(np.abs(t[tk]).max()) + 1e-6,
                  f"l{k} {key}")
        _half(_rel(rec["d_head"], t["grads"]["head"]), fx.tol("d_head"), f"l{k} d(loss)/d raw head")
        _half(_rel(rec["d_q"], t["grads"]["q"]), 1e-5, f"l{k} dQ")
        assert (float(rec["result/min_Q"]), float(rec["result/max_Q"])) == (float(rec["q"].min()), float(rec["q"].max())), "extrema over q [R]"
        assert (float(rec["result/min_At"]), float(rec["result/max_At"])) == (float(rec["At"].min()), float(rec["At"].max()))
        step = int(rec["mult0/eta/step"])
        assert step == k
        for j, n in enumerate(D.NAMES):
            assert int(rec[f"mult_grad/{n}/has_grad"]), f"{n}: all three multipliers have a gradient when the policy is continuous"
            x0, x1, g = float(rec[f"mult0/{n}"]), float(rec[f"mult1/{n}"]), float(rec[f"mult_grad/{n}"])
            _half(abs(t["mult_grads"][j] - g) / t["mult_scale"][j], 1e-5, f"l{k} d(loss)/d {n} against the magnitude of its terms")
            assert x1 == float(rec[f"result/{n}"]) and int(rec[f"mult1/{n}/step"]) == step + 1 and int(rec[f"mult1/{n}/has_state"])
            w, m, v = D.multiplier_step(x0, g, float(rec[f"mult0/{n}/exp_avg"]), float(rec[f"mult0/{n}/exp_avg_sq"]), step, fx.lr, fx.floors[j])
            _half(abs(x1 - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * fx.lr, f"l{k} {n} after its step")
            _half(abs(m - float(rec[f"mult1/{n}/exp_avg"])) / (abs(m) + 1e-30), 2e-5, f"l{k} {n} exp_avg")
            _half(abs(v - float(rec[f"mult1/{n}/exp_avg_sq"])) / (abs(v) + 1e-30), 2e-5, f"l{k} {n} exp_avg_sq")
        clip, clamp = D.distance_from_the_switches(t)
        assert clip > 1e-4 and clamp > 1e-4, "no row sits near the c = 1 clip or the +-5 clamp"


def test_fixtures_have_the_properties_the_issue_asks_for():
    fx = D.Fixture("mpo_cont")
    assert (fx.S, fx.A, fx.H, fx.B, fx.T, fx.R, fx.NS, fx.retrace, fx.learns) == (4, 3, 32, 5, 4, 20, 6, True, 2) and fx.mult == [2.0, pytest.approx(0.1), 0.5]
    for k in range(2):
        rec = fx.learn(k)
        done = rec["in_done"].reshape(fx.B, fx.T)
        assert done[:, : fx.T - 1].any(1).sum() >= 2 and done[:, fx.T - 2].any(), "done = 1 inside at least two trajectories, position T - 2 among them"
        assert (rec["c"] == 1.0).any() and (rec["c"] < 1.0).any(), "c is clipped in some rows and not in others"
        assert (np.abs(rec["in_action"]) == 1.0).any() and (np.abs(rec["head"][:, :3]) > 5.0).any() and not rec["d_head"][:, :3][np.abs(rec["head"][:, :3]) > 5.0].any()
        assert not np.array_equal(rec["qret0"], rec["qret"]) and not np.array_equal(rec["mu"], rec["mut"]) and not np.array_equal(rec["q"], rec["qt_a"])
    l0, l1 = fx.learn(0), fx.learn(1)
    assert float(l1["mult0/alpha_sigma"]) == float(l0["mult1/alpha_sigma"]) != float(l0["mult0/alpha_sigma"]) and int(l1["mult0/eta/step"]) == 1
    td = D.Fixture("mpo_cont_td")
    assert (td.A, td.T, td.NS, td.retrace, td.learns) == (1, 1, 1, False, 1)
    rec = td.learn(0)
    assert float(rec["mult1/alpha_sigma"]) == np.float32(td.floors[2]) and float(rec["mult_grad/alpha_sigma"]) > 0, "the clamped step of alpha_sigma"
    assert not rec["At"].any() and (rec["w"] == 1.0).all() and np.array_equal(rec["qret0"], rec["qret"]), "the degenerate E-step"
    pd = D.Fixture("mpo_cont_pendulum")
    assert (pd.S, pd.A, pd.H, pd.B, pd.T, pd.NS, pd.lr, pd.recipe, pd.NS * pd.R) == (3, 1, 512, 64, 4, 30, 2.5e-4, True, 7680)
    assert pd.learn(0)["eps"].shape == (2, 30, 256, 1), "the normals are stored whole: the tests inject them"
    for key in ("actor_loss", "eta_loss", "alpha_loss", "d_head", "At", "w"):
        assert float(pd.z[f"hyper/ref_{key}_err"]) < 1e-4, key
    for f in D.FIXTURES:
        assert os.path.getsize(os.path.join(D.GOLDEN, f + ".npz")) < (1 << 20)


def test_curve_fixture_is_the_reference_on_the_recorded_configuration():
    import json

    with open(os.path.join(D.GOLDEN, "curves_reference_mpo_continuous.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_mpo_continuous.py --only curves"
    curves = fx["mpo_control"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(curves) == 3 and all(len(c) * D.CURVE_CONFIG["bin"] == D.CURVE_CONFIG["steps"] for c in curves)
    tenths = [D.curve_tenths(c) for c in curves]
    assert all(np.isfinite(c).all() for c in curves) and all(0.05 < first < 0.15 for first, _ in tenths), "before learning starts the env pays about 0.1 per step"
    # the reference's own seeds end far apart on this env (one falls, two rise): that spread is what a HIP curve is compared to
    assert max(last for _, last in tenths) - min(last for _, last in tenths) > 0.5 and sum(last > first for first, last in tenths) >= 2
