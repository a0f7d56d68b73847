"""CPU-side checks of the Munchausen-DQN feature: the C ABI carries the new entries, the agent is registered under the reference's key,
the restatement in tests/mdqn_truth.py reproduces the reference's own learn() on the three fixtures (tools/gen_golden_mdqn.py), the
sweep's inputs have the properties the GPU test relies on, and configuration errors raise before any GPU use."""
import json
import os
import re

import numpy as np
import pytest
import torch

import mdqn_truth as M
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["mdqn", "mdqn_odd", "mdqn_cartpole"]
CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, hidden=512, batch=32, alpha=0.9, tau=0.03, l_0=-1, lr=1e-4, gamma=0.99,
                    epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_mdqn_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "m_dqn.py:" in src  # every declaration cites the reference lines it replaces
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("jh_mdqn_loss", "jh_rbnet_learn_forward_m", "jh_rbnet_reserve_target_rows"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2


def test_agent_is_registered_under_the_reference_key(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.mdqn import MDQN

    assert agent_dict["m_dqn"] is MDQN
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("m_dqn", state_size=4, action_size=2)


def test_configuration_errors_raise_before_any_gpu_use():
    from jorldy_amd.core.agent import Agent

    with pytest.raises(ValueError, match="libjorldy_hip") as e:
        Agent("m_dqn", state_size=4, action_size=2, network="rainbow")
    assert "rainbow" in str(e.value) and "discrete_q_network" in str(e.value)
    with pytest.raises(ValueError, match="tau=0"):
        Agent("m_dqn", state_size=4, action_size=2, tau=0)
    with pytest.raises(ValueError, match="tau=-0.03"):
        Agent("m_dqn", state_size=4, action_size=2, tau=-0.03)
    with pytest.raises(ValueError, match="l_0=0.5"):
        Agent("m_dqn", state_size=4, action_size=2, l_0=0.5)


def _fixture_truth(z, dtype):
    return M.mdqn_truth(z["learn/q_all"], z["learn/target_q_state"], z["learn/next_target_q"], z["learn/action"], z["learn/reward"], z["learn/done"],
                        float(z["hyper/gamma"]), float(z["hyper/alpha"]), float(z["hyper/m_tau"]), float(z["hyper/l_0"]), dtype)


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_truth_reproduces_the_reference_fixture(name):
    z = load(name)
    B, A = z["learn/q_all"].shape
    assert (B, A) == (int(z["hyper/B"]), int(z["hyper/A"]))
    assert (float(z["hyper/alpha"]), float(z["hyper/m_tau"]), float(z["hyper/l_0"])) == (0.9, 0.03, -1.0)
    t = _fixture_truth(z, torch.float32)
    np.testing.assert_allclose(t["target"], z["learn/target_q"].reshape(-1), rtol=1e-6)
    np.testing.assert_allclose(t["loss"], float(z["learn/loss"]), rtol=1e-6)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-6)
    np.testing.assert_allclose(t["max_Q"], float(z["result/max_Q"]), rtol=1e-6)
    ref = z["learn/d_q_all"]
    assert float(np.abs(t["grad"] - ref).max()) <= 1e-6 * float(np.abs(ref).max())
    np.testing.assert_allclose(t["mun_mean"], float(z["learn/munchausen_term"].mean()), rtol=1e-6)
    # the reference's own intermediates: the taken q, and a gradient that is zero off the taken action
    act = z["learn/action"].reshape(-1).astype(np.int64)
    np.testing.assert_array_equal(z["learn/q"].reshape(-1), z["learn/q_all"][np.arange(B), act])
    other = np.ones((B, A), bool)
    other[np.arange(B), act] = False
    assert not ref[other].any()
    # float64 stays close to it: what the GPU criterion max(1e-5, 2 x reference error) rests on
    t64 = _fixture_truth(z, torch.float64)
    assert abs(t64["loss"] - float(z["result/loss"])) <= 1e-6 * abs(t64["loss"])
    assert float(np.abs(t64["grad"] - ref).max()) <= 1e-6 * float(np.abs(t64["grad"]).max())


def test_online_and_target_weights_of_the_fixtures_differ():
    for name in ("mdqn", "mdqn_odd"):
        z = load(name)
        keys = [k[4:] for k in z.files if k.startswith("sd0/")]
        assert keys and all(not np.array_equal(z[f"sd0/{k}"], z[f"sdt/{k}"]) for k in keys)
        assert not np.array_equal(z["learn/q_all"], z["learn/target_q_state"])
    assert str(load("mdqn_odd")["hyper/network"]) == "dueling" and str(load("mdqn")["hyper/network"]) == "discrete_q_network"


def test_sweep_covers_the_boundaries_and_float32_stays_close_to_float64():
    """Properties of the GPU sweep's inputs, established here so that the GPU test may assert them: the reference's float32 arithmetic
    stays within 1e-6 (relative to max) of float64 on every case, so the 1e-5 criterion excludes nothing."""
    assert {c[0] for c in M.SWEEP} == {1, 7, 32, 255, 256, 257, 600}
    assert {c[1] for c in M.SWEEP} == {1, 2, 5, 6, 18}
    assert {c[2] for c in M.SWEEP} == {"plain", "wide", "flat", "tau1"}
    for B, A, variant in M.SWEEP:
        d, h = M.sweep_case(B, A, variant)
        t64, t32 = M.mdqn_truth(dtype=torch.float64, **d, **h), M.mdqn_truth(dtype=torch.float32, **d, **h)
        assert float(np.abs(t32["grad"] - t64["grad"]).max()) <= 1e-6 * float(np.abs(t64["grad"]).max()), (B, A, variant)
        assert abs(t32["loss"] - t64["loss"]) <= 1e-6 * abs(t64["loss"]), (B, A, variant)
        if A == 1:
            assert not t64["log_policy"].any() and not t32["log_policy"].any()
            np.testing.assert_allclose(t64["target"], d["reward"] + (1 - d["done"].astype(np.float64)) * h["gamma"] * d["q_next_target"][:, 0].astype(np.float64), rtol=1e-12)
        if variant == "flat":
            assert not t64["clipped"].any()
        if variant == "wide":
            assert t64["clipped"].any()
    for B, A in M.BOTH_SIDES:
        d, h = M.sweep_case(B, A, "plain")
        t = M.mdqn_truth(**d, **h)
        assert t["clipped"].any() and not t["clipped"].all(), (B, A)
        assert t["linear"].any() and not t["linear"].all(), (B, A)


def test_curve_fixture_was_made_with_the_config_the_gpu_test_runs():
    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_mdqn.json")) as f:
        fx = json.load(f)
    assert fx["mdqn_cartpole"]["config"] == CURVE_CONFIG
    ref = fx["mdqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == CURVE_CONFIG["steps"] // CURVE_CONFIG["chunk"] for r in ref)
    # the DQN curve test's assertions hold for the reference's own three seeds: the GPU test keeps all three
    start, end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    assert start < 40 and end > 4 * start
