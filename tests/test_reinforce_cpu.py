"""CPU-side checks of the REINFORCE feature: the C ABI carries the three new entries, the agent is registered under the reference's key and fails
loudly without a GPU, configurations outside the native engine raise at construction, the float64 statement in tests/reinforce_truth.py reproduces
the reference's own learn() on the recorded tensors of the fixtures (tools/gen_golden_reinforce.py) at half the tolerances the GPU tests give the
kernels, the Gaussian policy's key table round-trips, and the properties of the fixtures and case builders that the GPU tests rely on."""
import json
import os
import re

import numpy as np
import pytest
import torch

import reinforce_truth as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("jh_reinforce_returns", "jh_reinforce_loss_discrete", "jh_reinforce_loss_continuous")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_new_entries(lib):
    from jorldy_amd import _lib, ops

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "reinforce.py:83-113" in src and "policy.py:49-55" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2
    assert ops.REINFORCE_MAX_ROWS == D.MAX_ROWS == 65536
    assert "jh_reinforce.hip" in open(os.path.join(ROOT, "jorldy_amd", "csrc", "Makefile")).read()


def test_agent_is_registered_and_fails_loudly_without_a_gpu(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.reinforce import REINFORCE

    assert agent_dict["reinforce"] is REINFORCE
    if not torch.cuda.is_available():
        for kw in (dict(), dict(network="continuous_policy", action_size=1), dict(head="cnn", state_size=(4, 84, 84)), dict(row_capacity=8), dict(some_unknown_keyword=1),
                   dict(optim_config={"name": "adam", "lr": 1e-4}, gamma=0.99, lr_decay=True)):  # the last: config.reinforce.cartpole
            base = dict(state_size=4, action_size=2)
            base.update(kw)
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                Agent("reinforce", **base)


@pytest.mark.parametrize("kw", [dict(network="discrete_policy_value"), dict(network="deterministic_policy"), dict(head="multi"), dict(head="cnn"),
                                dict(head="cnn", state_size=(4, 20, 20)), dict(optim_config={"name": "rmsprop"}), dict(optim_config={"name": "adam", "weight_decay": 0.1}),
                                dict(hidden_size=30), dict(action_size=1), dict(action_size=65), dict(network="continuous_policy", action_size=0),
                                dict(network="continuous_policy", action_size=33), dict(grad_sync=object()), dict(row_capacity=0)],
                         ids=["policy_value", "deterministic", "multi_head", "cnn_scalar_state", "cnn_small_frames", "rmsprop", "weight_decay", "hidden_30", "A_1", "A_65",
                              "cont_A_0", "cont_A_33", "grad_sync", "row_capacity_0"])
def test_configurations_outside_the_native_engine_raise_at_construction(kw):
    """Before any GPU use: the check comes ahead of the device check, so it holds on every machine."""
    from jorldy_amd.core.agent import Agent

    base = dict(state_size=4, action_size=2)
    base.update(kw)
    with pytest.raises(ValueError, match="REINFORCE runs on libjorldy_hip only") as e:
        Agent("reinforce", **base)
    for word in ("discrete_policy", "continuous_policy", "multi", "grad_sync", "hidden_size % 4 == 0", "adam"):
        assert word in str(e.value), word


# ---------------------------------------------------------------------------------------------- the truth
def test_truth_scan_is_the_python_loop_over_all_rows_in_float64():
    """The recurrence written out row by row in float64 (what reinforce.py:90-92 does to a float64 reward column), against D.scan bit for bit; and
    against the closed form sum_k gamma^k r[t + k] at a small T."""
    rs = np.random.RandomState(0)
    for T in (1, 2, 9, 37, 500):
        for gamma in (0.99, 1.0, 0.5):
            r = rs.randn(T).astype(np.float32)
            ret = r.astype(np.float64)
            t = T - 2
            while t >= 0:
                ret[t] += gamma * ret[t + 1]
                t -= 1
            assert np.array_equal(D.scan(r, gamma), ret), (T, gamma)
            if T <= 37:
                closed = np.asarray([sum(gamma ** k * float(r[t + k]) for k in range(T - t)) for t in range(T)])
                assert np.abs(closed - ret).max() <= 1e-12 * np.abs(ret).max()
            s = D.returns(r, gamma, True)
            if T == 1:
                assert s[0] == 0.0, "one row standardises to exactly 0"
            else:
                assert abs(s.mean()) < 1e-12 and abs(s.std() - 1.0) < 1e-5


def _half(err, tol, what):
    assert err <= 0.5 * tol, f"{what}: {err:.3e} is more than half of the GPU test's tolerance {tol:.3e}"


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    """Float64 against the reference's own run, every learn, each achieved value at no more than half of the GPU test's tolerance: `ret` by the
    scan test's per-element bound around the recorded value (2^-23 |ret| + 1e-6 max |ret|), the loss rtol 1e-5, the head gradient 1e-5 of the
    tensor's largest entry; the torch restatement in float64 agrees with the numpy statement."""
    fx = D.load_fixture(name)
    for k in range(fx.learns):
        rec = fx.learn(k)
        T = fx.rows[k]
        assert rec["in/reward"].shape == (T, 1) and bool(rec["in/done"][-1, 0]) and not rec["in/done"][:-1].any(), "one episode: only its last row is done"
        ret = D.returns(rec["in/reward"].astype(np.float32), fx.gamma, fx.standardize)
        ref = rec["ret"].astype(np.float64)
        bound = 2.0 ** -23 * np.abs(ref) + 1e-6 * np.abs(ref).max()
        _half(float((np.abs(ret - ref) / bound).max()), 1.0, f"l{k} ret, as a fraction of the per-element bound")
        t = D.case_truth(fx.kind, dict(head=rec["out"], action=rec["in/action"], ret=rec["ret"]))
        _half(abs(t["loss"] - float(rec["loss"])) / abs(float(rec["loss"])), 1e-5, f"l{k} loss")
        g = rec["d_out"].astype(np.float64)
        _half(float(np.abs(t["grad"] - g).max() / np.abs(g).max()), 1e-5, f"l{k} d(loss)/d(head)")
        _half(float(np.abs(t["logp"].reshape(rec["log_prob"].shape) - rec["log_prob"]).max() / np.abs(rec["log_prob"]).max()), 1e-5, f"l{k} log_prob")
        t64 = D.loss_torch(fx.kind, rec["out"], rec["in/action"], rec["ret"], torch.float64)
        assert abs(t64["loss"] - t["loss"]) <= 1e-12 * abs(t["loss"])
        assert np.abs(t64["grad"] - t["grad"]).max() <= 1e-12 * np.abs(t["grad"]).max() + 1e-18
        assert int(rec["opt/step"]) == k + 1
        assert float(rec["lr"]) == fx.lr * float(np.cos(0.5 * np.pi * int(rec["steps"][-1]) / fx.run_step)), "the cosine decay at the episode's last step"


def test_fixtures_have_the_properties_the_issue_asks_for():
    d = D.load_fixture("reinforce_discrete")
    assert (d.S, d.A, d.H, d.rows, d.cont, d.standardize) == (4, 3, 64, [37, 12], False, True)
    c = D.load_fixture("reinforce_continuous")
    assert (c.S, c.A, c.H, c.rows, c.cont) == (5, 3, 32, [29, 50], True)
    for k in range(2):
        rec = c.learn(k)
        mu_raw = rec["out"][:, : c.A]
        assert (np.abs(rec["in/action"]) == 1.0).any(), "a stored action is exactly +-1.0"
        assert (np.abs(mu_raw) > 5.0).any() and (np.abs(mu_raw) < 5.0).any(), "mu_raw on both sides of the clamp"
        assert not rec["d_out"][:, : c.A][np.abs(mu_raw) > 5.0].any() and np.isfinite(rec["d_out"]).all(), "no gradient through a clamped mu_raw"
        assert list(rec["steps"]) == list(range(1 + 29 * k, 1 + 29 * k + c.rows[k]))
    n = D.load_fixture("reinforce_nostd")
    assert (n.rows, n.standardize, n.gamma) == ([9], False, 1.0)
    rec = n.learn(0)
    assert np.array_equal(rec["ret"], np.cumsum(rec["in/reward"][::-1, 0])[::-1].astype(np.float32)), "gamma 1 without standardisation: plain suffix sums"
    cp = D.load_fixture("reinforce_cartpole")
    assert (cp.S, cp.A, cp.H, cp.lr, cp.gamma, cp.run_step, cp.recipe, cp.learns) == (4, 2, 512, 1e-4, 0.99, 100000, True, 1)
    rec = cp.learn(0)
    assert np.allclose(rec["in/reward"][:-1], 0.1) and float(rec["in/reward"][-1, 0]) == -1.0, "a real CartPole episode of the oracle's"
    assert [tuple(v.shape) for v in cp.sd0().values()] == [(512, 4), (512,), (512, 512), (512,), (2, 512), (2,)]
    for f in D.FIXTURES:
        assert os.path.getsize(os.path.join(D.GOLDEN, f + ".npz")) < (1 << 20)
        fx = D.load_fixture(f)
        for k in range(fx.learns):  # the generator's condition: the recorded loss is a well-conditioned sum (tools/gen_golden_reinforce.py)
            rec = fx.learn(k)
            terms = rec["log_prob"].astype(np.float64).reshape(fx.rows[k], -1) * rec["ret"].astype(np.float64).reshape(-1, 1)
            assert np.abs(terms).sum() / abs(terms.sum()) <= float(fx.z["hyper/max_kappa"]) == 64.0, (f, k)


def test_curve_fixture_is_the_reference_on_the_recorded_configuration():
    with open(os.path.join(D.GOLDEN, "curves_reference_reinforce.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_reinforce.py --only curves"
    c = fx["config"]
    assert c["agent"]["optim_config"]["lr"] == 1e-3 and 20000 <= c["steps"] <= 30000 and c["agent"]["hidden_size"] == 512
    curves = fx["reinforce_cartpole"]["reference"]
    assert len(curves) == 3 and all(len(v) * c["chunk"] == c["steps"] for v in curves)
    tenths = [D.curve_tenths(v) for v in curves]
    assert fx["search"][-1]["steps"] == c["steps"] and fx["search"][-1]["first_last_tenths"] == [list(t) for t in tenths]
    assert fx["accepted"] == all(last >= 2.0 * first for first, last in tenths)
    assert all(not s["accepted"] for s in fx["search"][:-1]), "the smallest accepted budget is the one kept"


# ---------------------------------------------------------------------------------------------- the case builders
def test_no_sweep_case_sits_on_a_discontinuity():
    """The continuous loss has two kinks: the clamp of mu_raw at +-5 (its gradient jumps) and the clamp of the action at the float32 bound.  Every
    |mu_raw| of every sweep case is at least 1e-3 away from 5, and no |action| lies strictly between the float32 clamp bound and 1."""
    bound = np.float32(D.CLAMP_HI)
    assert bound == np.float32(1 - 1e-7) and np.nextafter(bound, np.float32(2)) != np.float32(1.0), "there ARE float32 values between the bound and 1"
    for T in D.LOSS_T:
        for A in D.LOSS_A["continuous"]:
            c = D.loss_case("continuous", T, A)
            mu_raw = c["head"][:, :A]
            assert c["head"].shape == (T, 2 * A) and c["action"].shape == (T, A) and c["head"].dtype == c["action"].dtype == np.float32
            assert np.abs(np.abs(mu_raw) - 5.0).min() >= 1e-3, (T, A)
            a = np.abs(c["action"])
            assert not ((a > bound) & (a < 1.0)).any() and a.max() == 1.0, (T, A)
            assert (np.abs(mu_raw) > 5.0).any(), "a clamped mu_raw in every case"
            t = D.case_truth("continuous", c)
            assert np.isfinite(t["grad"]).all() and np.isfinite(t["loss"]) and not t["grad"][:, :A][np.abs(mu_raw) > 5.0].any()
    for T in D.LOSS_T:
        for A in D.LOSS_A["discrete"]:
            c = D.loss_case("discrete", T, A)
            assert c["head"].shape == (T, A) and 0 <= c["action"].min() and c["action"].max() <= A - 1
            t = D.case_truth("discrete", c)
            assert np.abs(t["grad"].sum(1)).max() <= 1e-15 * max(1.0, np.abs(c["ret"]).max()), "row sums of the discrete gradient vanish"


def test_every_standardised_sweep_case_has_a_standard_deviation_far_above_the_1e_7():
    """std >= 1e-3 max |ret| in every standardised case with more than one row: the + 1e-7 of the denominator is not what the sweep tests.
    (T = 1 standardises to exactly 0 whatever the denominator.)"""
    assert set((1, 2, 63, 64, 65, 1023, 1024, 1025, 65536)) <= set(D.RETURN_T) and set(D.RETURN_GAMMA) == {0.99, 1.0, 0.5}
    n = 0
    for T, gamma, standardize, kind in D.return_cases():
        if not standardize or T == 1:
            continue
        ret = D.scan(D.reward_case(T, kind), gamma)
        assert ret.std() >= 1e-3 * np.abs(ret).max(), (T, gamma, kind)
        n += 1
    assert n == (len(D.RETURN_T) - 1) * 3 * 2


def test_gauss_key_table_round_trips_through_a_continuous_policy_state_dict():
    """The Gaussian policy is a q-network with 2A output rows (core/network/policy.py:38-55): RainbowNet(kind="gauss")'s key table against a torch
    module of that shape, names, shapes and order."""
    from jorldy_amd import ops
    from jorldy_amd.core.network import Network

    torch.manual_seed(3)
    S, H, A = 5, 32, 3
    pol = Network("continuous_policy", S, A, D_hidden=H, head="mlp")
    assert list(pol.state_dict()) == ["head.l.weight", "head.l.bias", "l.weight", "l.bias", "mu.weight", "mu.bias", "log_std.weight", "log_std.bias"]

    class _Net(ops.RainbowNet):  # the key table alone: no device, no library
        def __init__(self):
            self.kind, self.cnn, self.H, self.A, self.n_actions = "gauss", False, H, 2 * A, A
            up4 = lambda n: (n + 3) // 4 * 4
            self.seg, off = {}, 0
            for name, rows, cols in (("w1", H, S), ("b1", 1, H), ("wl", H, H), ("bl", 1, H), ("mu_a2", 2 * A, H), ("mub_a2", 1, 2 * A)):
                self.seg[name] = (off, rows, cols)
                off += up4(rows * cols)
            self.n = off
            self.device = torch.device("cpu")

        def __del__(self):
            pass

    net = _Net()
    bucket = torch.zeros(net.n)
    net.import_state(pol.state_dict(), bucket)
    back = net.export_state(bucket)
    assert list(back) == list(pol.state_dict())
    for k, v in pol.state_dict().items():
        assert torch.equal(back[k], v), k
    w = net._v(bucket, "mu_a2")
    assert torch.equal(w[:A], pol.mu.weight.detach()) and torch.equal(w[A:], pol.log_std.weight.detach()), "ONE last layer: mu's rows, then log_std's"
    Network("continuous_policy", S, A, D_hidden=H, head="mlp").load_state_dict(back)  # strict: names and shapes are torch's own
