"""CPU-side checks of the MPO feature: the C ABI carries the new entries, the agent is registered under the reference's key and fails loudly without
a GPU, configurations outside the native engine raise at construction, the float64 statement in tests/mpo_truth.py reproduces the reference's own
learn() on every recorded tensor of the fixtures (tools/gen_golden_mpo.py) at half the tolerances the GPU tests give the kernel (those of
tests/test_vmpo_cpu.py for the same comparison), the pi.* / q.* key mapping round-trips, interact_callback's window, and the properties of the
fixtures and case builders that the GPU tests rely on."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mpo_truth as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("jh_mpo_loss_discrete", "jh_rbnet_learn_forward_p", "jh_rbnet_hyper_ptr")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_new_entries(lib):
    from jorldy_amd import _lib, ops

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "mpo.py:312-386" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert ops.MPO_STATS == D.STATS and len(D.STATS) == 11
    # ONE copy of the multiplier step: the header both kernels include
    csrc = os.path.join(ROOT, "jorldy_amd", "csrc")
    for f in ("jh_vmpo.hip", "jh_mpo.hip"):
        s = open(os.path.join(csrc, f)).read()
        assert '#include "jh_mult.h"' in s and "float multiplier_step(" not in s
    assert "float multiplier_step(" in open(os.path.join(csrc, "jh_mult.h")).read()


def test_agent_is_registered_and_fails_loudly_without_a_gpu(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.mpo import MPO

    assert agent_dict["mpo"] is MPO
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("mpo", state_size=4, action_size=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("mpo", state_size=4, action_size=2, batch_size=128, n_step=8, some_unknown_keyword=1)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("mpo", state_size=4, action_size=2, batch_size=1024, n_step=8, critic_loss_type="1step_TD")  # n_step counts as 1


@pytest.mark.parametrize("kw", [dict(actor="continuous_policy", critic="continuous_q_network"), dict(actor="continuous_policy"), dict(head="cnn", state_size=(4, 84, 84)),
                                dict(batch_size=129, n_step=8), dict(batch_size=1025, critic_loss_type="1step_TD"), dict(hidden_size=30),
                                dict(optim_config={"name": "rmsprop"}), dict(optim_config={"name": "adam", "weight_decay": 0.1}), dict(action_size=1), dict(action_size=65),
                                dict(critic="dueling"), dict(critic_loss_type="td_lambda"), dict(grad_sync=object())],
                         ids=["continuous", "continuous_actor", "cnn", "rows_1032", "td_rows_1025", "hidden_30", "rmsprop", "weight_decay", "A_1", "A_65", "dueling_critic",
                              "loss_type", "grad_sync"])
def test_configurations_outside_the_native_engine_raise_at_construction(kw):
    """Before any GPU use: the check comes ahead of the device check, so it holds on every machine."""
    from jorldy_amd.core.agent import Agent

    base = dict(state_size=4, action_size=2)
    base.update(kw)
    with pytest.raises(ValueError, match="MPO runs on libjorldy_hip only") as e:
        Agent("mpo", **base)
    for word in ("discrete_policy", "discrete_q_network", "continuous_policy", "cnn", "grad_sync", "batch_size \\* n_step <= 1024"):
        assert re.search(word, str(e.value)), word


def _half(err, tol, what):
    assert err <= 0.5 * tol, f"{what}: {err:.3e} is more than half of the GPU test's tolerance {tol:.3e}"


def _rel(a, b):
    return abs(float(a) - float(b)) / (abs(float(b)) + 1e-30)


def _truth_of(fx, rec):
    mult0 = [float(rec[f"mult0/{n}"]) for n in D.NAMES]
    return D.loss(rec["la"], rec["la_next"], rec["la_old"], rec["q"], rec["qt"], rec["qt_next"], rec["in_action"], rec["in_reward"], rec["in_done"], rec["in_prob"],
                  fx.T, mult0, fx.eps, fx.gamma, fx.retrace), mult0


def _with_inputs(fx, rec):
    rows = fx.replay()
    for key in ("action", "reward", "done", "prob"):
        rec["in_" + key] = np.concatenate([rows[i][key] for i in rec["idx"]], 0).reshape(-1).astype(np.float32)
    return rec


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    """Float64 against the reference's float32 run, every learn, each achieved value at no more than half of the GPU test's tolerance: the four
    losses rtol 1e-5, c, Qret before and after the scan, At and the E-step weights 1e-5 of the tensor's largest entry, head gradients 1e-5 of the
    largest entry, the multipliers' gradients 1e-5 of the magnitude of their terms (they are differences), the multipliers after their step by
    fp64_truth's per-element criterion, their moments 2e-5; the extrema in `result` bit for bit from the recorded tensors."""
    fx = D.load_fixture(name)
    assert fx.R == fx.B * fx.T <= 1024
    for k in range(fx.learns):
        rec = _with_inputs(fx, fx.learn(k))
        t, mult0 = _truth_of(fx, rec)
        for key, ref in (("actor", "actor_loss"), ("critic", "critic_loss"), ("eta_loss", "eta_loss"), ("alpha_loss", "alpha_loss")):
            _half(_rel(t[key], rec[ref]), 1e-5, f"l{k} {ref}")
            assert float(rec[ref]) == float(rec[f"result/{ref}"])
        for key in ("c", "qret0", "qret", "At", "w"):
            ref = rec[key].astype(np.float64).reshape(t[key].shape)
            _half(float(np.abs(t[key] - ref).max() / np.abs(ref).max()), 1e-5, f"l{k} {key}")
        for key in ("la", "q"):
            ref = rec[f"d_{key}"].astype(np.float64)
            _half(float(np.abs(t["grads"][key] - ref).max() / np.abs(ref).max()), 1e-5, f"l{k} d(loss)/d {key}")
        a = rec["in_action"].astype(np.int64)
        other = np.ones_like(rec["d_q"], dtype=bool)
        other[np.arange(fx.R), a] = False
        assert not rec["d_q"][other].any() and not t["grads"]["q"][other].any()
        assert (float(rec["result/min_Q"]), float(rec["result/max_Q"])) == (float(rec["q"].min()), float(rec["q"].max())), "extrema over ALL of q [R, A]"
        assert (float(rec["result/min_At"]), float(rec["result/max_At"])) == (float(rec["At"].min()), float(rec["At"].max()))
        step = int(rec["mult0/eta/step"])
        assert step == k
        for j, n in enumerate(D.NAMES):
            has_grad = bool(int(rec[f"mult_grad/{n}/has_grad"]))
            assert has_grad == (t["mult_grads"][j] is not None) == (n != "alpha_sigma"), (n, "alpha_sigma has no gradient when the policy is discrete")
            x0, x1 = float(rec[f"mult0/{n}"]), float(rec[f"mult1/{n}"])
            assert x1 == float(rec[f"result/{n}"])
            if not has_grad:  # torch's Adam skips it: no state, value unchanged
                assert x1 == x0 and not int(rec[f"mult1/{n}/has_state"])
                continue
            g = float(rec[f"mult_grad/{n}"])
            _half(abs(t["mult_grads"][j] - g) / t["mult_scale"][j], 1e-5, f"l{k} d(loss)/d {n} against the magnitude of its terms")
            assert int(rec[f"mult1/{n}/step"]) == step + 1 and int(rec[f"mult1/{n}/has_state"])
            w, m, v = D.multiplier_step(x0, g, float(rec[f"mult0/{n}/exp_avg"]), float(rec[f"mult0/{n}/exp_avg_sq"]), step, fx.lr, fx.floors[j])
            _half(abs(x1 - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * fx.lr, f"l{k} {n} after its step")
            _half(_rel(m, rec[f"mult1/{n}/exp_avg"]), 2e-5, f"l{k} {n} exp_avg")
            _half(_rel(v, rec[f"mult1/{n}/exp_avg_sq"]), 2e-5, f"l{k} {n} exp_avg_sq")
        # the torch restatement in float64 agrees with the numpy statement (it is the float32 comparator of the GPU tests)
        t64 = D.loss_torch(rec["la"], rec["la_next"], rec["la_old"], rec["q"], rec["qt"], rec["qt_next"], rec["in_action"], rec["in_reward"], rec["in_done"],
                           rec["in_prob"], fx.T, mult0, fx.eps, fx.gamma, fx.retrace, torch.float64)
        for key in ("actor", "critic", "eta_loss", "alpha_loss"):
            assert _rel(t64[key], t[key]) <= 1e-12, key
        for key in ("la", "q"):
            assert np.abs(t64["grads"][key] - t["grads"][key]).max() <= 1e-12 * np.abs(t["grads"][key]).max() + 1e-18
        for j in range(2):
            assert abs(t64["mult_grads"][j] - t["mult_grads"][j]) <= 1e-12 * t["mult_scale"][j]


def test_fixtures_have_the_properties_the_issue_asks_for():
    fx = D.load_fixture("mpo_discrete")
    assert (fx.S, fx.A, fx.H, fx.B, fx.T, fx.R, fx.retrace, fx.learns) == (4, 3, 32, 5, 4, 20, True, 2) and fx.mult == [2.0, pytest.approx(0.1), 1.0]
    rows = fx.replay()
    for key in D.COLUMNS:
        assert np.array_equal(np.concatenate([r[key] for r in rows], 0), fx.z[f"in/{key}"]), f"the replay recipe regenerates the stored column {key}"
    for k in range(2):
        rec = _with_inputs(fx, fx.learn(k))
        done = rec["in_done"].reshape(fx.B, fx.T)
        assert done[:, : fx.T - 1].any(1).sum() >= 2 and done[:, fx.T - 2].any(), "done = 1 inside at least two trajectories, position T - 2 among them"
        assert (rec["c"] == 1.0).any() and (rec["c"] < 1.0).any(), "c is clipped in some rows and not in others"
        assert not np.array_equal(rec["qret0"], rec["qret"])
    l0, l1 = fx.learn(0), fx.learn(1)
    assert float(l1["mult0/eta"]) == float(l0["mult1/eta"]) != float(l0["mult0/eta"]) and int(l1["mult0/eta/step"]) == 1, "the one-step lag of the multipliers"
    assert not np.array_equal(l0["la"], l0["la_old"]) and not np.array_equal(l0["q"], l0["qt"]), "the targets differ from their online nets"
    td = D.load_fixture("mpo_td")
    assert (td.A, td.T, td.retrace, td.learns) == (2, 1, False, 1)
    rec = td.learn(0)
    assert float(rec["mult1/eta"]) == np.float32(td.floors[0]) and float(rec["mult0/eta"]) - td.lr < td.floors[0] and float(rec["mult_grad/eta"]) > 0, "the clamped step"
    assert np.array_equal(rec["qret0"], rec["qret"])
    cp = D.load_fixture("mpo_cartpole")
    assert (cp.S, cp.A, cp.H, cp.B, cp.T, cp.lr, cp.recipe) == (4, 2, 512, 64, 4, 2.5e-4, True)
    for f in D.FIXTURES:
        assert os.path.getsize(os.path.join(D.GOLDEN, f + ".npz")) < (1 << 20)


def test_curve_fixture_is_the_reference_on_the_recorded_configuration():
    with open(os.path.join(D.GOLDEN, "curves_reference_mpo.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_mpo.py --only curves"
    curves = fx["mpo_cartpole"]["reference"]
    assert len(curves) == 3 and all(len(c) * fx["bin"] == D.CURVE_CONFIG["steps"] for c in curves)
    for c in curves:
        first, last = D.curve_tenths(c)
        # reward is 0.1 per step and -1 at an episode end: a mean reward per step r stands for a mean episode length 1.1 / (0.1 - r)
        assert last > first and 1.1 / (0.1 - last) >= 1.5 * 1.1 / (0.1 - first), "the reference itself learns: episodes of the last tenth at least half as long again"


def test_policy_key_mapping_round_trips_through_a_discrete_policy_state_dict():
    """The actor is a q-network whose last layer is called pi (core/network/policy.py:23-35): RainbowNet(kind="pi")'s key table against a torch module
    of that shape, names, shapes and order; the critic keeps q.*."""
    from jorldy_amd import ops
    from jorldy_amd.core.network import DiscretePolicy, DiscreteQ_Network, Network, network_dict

    assert network_dict["discrete_policy"] is DiscretePolicy
    torch.manual_seed(3)
    pol, qn = Network("discrete_policy", 4, 3, D_hidden=32, head="mlp"), Network("discrete_q_network", 4, 3, D_hidden=32, head="mlp")
    assert list(pol.state_dict()) == ["head.l.weight", "head.l.bias", "l.weight", "l.bias", "pi.weight", "pi.bias"]
    assert [k.replace("pi.", "q.") for k in pol.state_dict()] == list(qn.state_dict()) and isinstance(qn, DiscreteQ_Network)
    assert float(pol.pi.weight.detach().abs().max()) < 0.02 < float(qn.q.weight.detach().abs().max()), "the policy gain 0.01 against the linear gain 1"

    class _Net(ops.RainbowNet):  # the key table alone: no device, no library
        def __init__(self, kind, S, H, A):
            self.kind, self.cnn, self.H, self.A = kind, False, H, A
            up4 = lambda n: (n + 3) // 4 * 4
            self.seg, off = {}, 0
            for name, rows, cols in (("w1", H, S), ("b1", 1, H), ("wl", H, H), ("bl", 1, H), ("mu_a2", A, H), ("mub_a2", 1, A)):
                self.seg[name] = (off, rows, cols)
                off += up4(rows * cols)
            self.n = off
            self.device = torch.device("cpu")

        def __del__(self):
            pass

    for kind, module in (("pi", pol), ("q", qn)):
        net = _Net(kind, 4, 32, 3)
        bucket = torch.zeros(net.n)
        net.import_state(module.state_dict(), bucket)
        back = net.export_state(bucket)
        assert list(back) == list(module.state_dict())
        for k, v in module.state_dict().items():
            assert torch.equal(back[k], v), k
        fresh = type(module)(4, 3, D_hidden=32, head="mlp")
        fresh.load_state_dict(back)  # strict: names and shapes are torch's own


def test_interact_callback_emits_nothing_until_the_window_is_full():
    from jorldy_amd.core.agent.mpo import MPO

    for loss_type, n_step, T in (("retrace", 4, 4), ("1step_TD", 4, 1)):
        agent = MPO.__new__(MPO)  # the window alone: no device
        from collections import deque

        agent.n_step = n_step if loss_type == "retrace" else 1
        agent.tmp_buffer = deque(maxlen=agent.n_step)
        outs = []
        for i in range(7):
            tr = {"state": np.full((1, 4), i, np.float32), "action": np.asarray([[i % 2]]), "reward": np.asarray([[0.1]]), "next_state": np.full((1, 4), i + 1, np.float32),
                  "done": np.asarray([[i == 2]]), "prob": np.asarray([[0.5]], np.float32)}
            outs.append(agent.interact_callback(tr))
        assert [bool(o) for o in outs] == [i >= T - 1 for i in range(7)]
        full = outs[-1]
        assert {k: v.shape for k, v in full.items()} == {"state": (1, T, 4), "action": (1, T, 1), "reward": (1, T, 1), "next_state": (1, T, 4), "done": (1, T, 1),
                                                         "prob": (1, T, 1)}
        assert full["state"][0, :, 0].tolist() == list(range(7 - T, 7)), "a sliding window: consecutive emissions overlap"
        if T == 4:
            assert outs[3]["done"][0, :, 0].tolist() == [False, False, True, False], "windows straddle episode ends"


def test_case_builders_have_the_properties_the_gpu_tests_rely_on():
    assert [b * t for b, t, _ in D.KERNEL_CASES] == [3, 20, 128, 264, 1024, 1]
    for B, T, A in D.KERNEL_CASES:
        c = D.case(B, T, A)
        t = D.case_truth(c)
        if T > 1:
            assert c["done"].reshape(B, T)[:, : T - 1].any() and c["done"][T - 2] == 1.0, "a done inside a trajectory, at the position the scan's mask reads last"
            assert not np.array_equal(t["qret0"], t["qret"]) and np.array_equal(D.case_truth(c, retrace=False)["qret"], t["qret0"])
        if B * T >= 3:
            assert (t["c"] == 1.0).any() and (t["c"] < 1.0).any(), "prob_b on both sides of the clip"
    c = D.case(16, 8, 2, "hot")
    t64, t32 = D.case_truth(c), D.case_truth(c, dtype=torch.float32)
    assert float(np.abs(t64["At"]).max()) / 1e-3 > 100.0
    assert np.isfinite(t64["eta_loss"]) and np.isfinite(t64["mult_grads"][0]) and not np.isfinite(t32["eta_loss"]), "float64 around the row maximum holds, float32 exp overflows"
    c = D.case(5, 4, 3, "floor")
    t = D.case_truth(c)
    for j in range(2):
        w, _, _ = D.multiplier_step(c["mult"][j], t["mult_grads"][j], c["m"][j], c["v"][j], D.STEP0, D.LR, c["floors"][j], D.BETAS, D.ADAM_EPS)
        assert w == float(c["floors"][j]), f"the step of {D.NAMES[j]} crosses its floor"
