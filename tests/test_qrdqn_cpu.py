"""CPU-side checks of the QR-DQN feature: the C ABI carries the two new entries, the agent is registered, the float64 truth of
tests/qr_truth.py reproduces the reference's own learn() on the three fixtures (tools/gen_golden_qrdqn.py), and the agent's host-side
tau is the reference's bit for bit."""
import os
import re

import numpy as np
import pytest

import qr_truth as Q
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["qrdqn", "qrdqn_odd", "qrdqn_cartpole"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_qr_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "qrdqn.py:" in src  # every declaration cites the reference lines it replaces
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("jh_qr_loss", "jh_quantile_act"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2


def test_agent_is_registered_and_fails_without_a_gpu_like_the_others(lib):
    import torch

    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.qrdqn import QRDQN

    assert agent_dict["qrdqn"] is QRDQN
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Agent("qrdqn", state_size=4, action_size=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Agent("dqn", state_size=4, action_size=2)


def test_configuration_errors_name_the_library_and_what_is_eligible():
    from jorldy_amd.core.agent import Agent

    with pytest.raises(ValueError, match="libjorldy_hip") as e:
        Agent("qrdqn", state_size=4, action_size=2, network="dueling")
    assert "discrete_q_network" in str(e.value)
    with pytest.raises(ValueError, match="98"):
        Agent("qrdqn", state_size=4, action_size=2, num_support=98)


def _fixture_truth(z):
    N = int(z["tau"].size)
    B = int(z["learn/logit"].shape[0])
    lg = [z[f"learn/{k}"].reshape(B, -1, N) for k in ("logit", "logit_next", "logit_target")]
    return Q.qr_truth(lg[0], lg[1], lg[2], z["learn/action"], z["learn/reward"], z["learn/done"], z["tau"], float(z["hyper/gamma"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    z = load(name)
    t = _fixture_truth(z)
    np.testing.assert_allclose(t["loss"], float(z["learn/loss"]), rtol=1e-6)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-6)
    ref = z["learn/d_logit"].astype(np.float64)
    err = float(np.abs(t["grad"].reshape(ref.shape) - ref).max())
    assert err <= 1e-6 * float(np.abs(ref).max()), err
    assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(-1).astype(np.int64))
    for k in ("max_Q", "max_logit", "min_logit"):
        np.testing.assert_allclose(t[k], float(z[f"result/{k}"]), rtol=1e-6, err_msg=k)
    # the reference's own intermediate tensors (index i = prediction, j = target)
    B, N = ref.shape[0], int(z["tau"].size)
    act = z["learn/action"].reshape(-1).astype(np.int64)
    np.testing.assert_array_equal(z["learn/theta_pred"].reshape(B, N), z["learn/logit"].reshape(B, -1, N)[np.arange(B), act])
    # no row of a fixture has its two best next actions closer than two fp32 sums of N terms can be off by
    assert int((t["gap"] <= t["gap_bound"]).sum()) == 0


@pytest.mark.parametrize("name", FIXTURES)
def test_host_tau_equals_the_fixture_bit_for_bit(name):
    from jorldy_amd.core.agent.qrdqn import quantile_midpoints

    z = load(name)
    tau = quantile_midpoints(int(z["hyper/num_support"])).numpy()
    assert tau.dtype == np.float32 and np.array_equal(tau.view(np.uint32), z["tau"].astype(np.float32).view(np.uint32))


def test_bad_num_support_raises():
    from jorldy_amd.core.agent.qrdqn import quantile_midpoints

    with pytest.raises(ValueError, match="99 elements"):
        quantile_midpoints(98)
    for n in (1, 8, 21, 33, 51, 64, 65, 200, 256):
        assert quantile_midpoints(n).numel() == n


def test_sweep_inputs_cover_every_size_and_leave_few_near_ties():
    """The GPU sweep compares the selected action through the loss on rows whose two best quantile means of online(s') are further
    apart than 2 N 2^-24 max|logit| (two fp32 sums of N terms); at most 1 % of a case's rows may fall under that."""
    from jorldy_amd.core.agent.qrdqn import quantile_midpoints

    assert {c[0] for c in Q.SWEEP} == {1, 3, 32, 255, 512, 1030}
    assert {c[1] for c in Q.SWEEP} == {1, 2, 6, 18}
    assert {c[2] for c in Q.SWEEP} == {1, 8, 51, 64, 65, 200, 256}
    assert (32, 18, 200, "plain") in Q.SWEEP and (512, 6, 200, "plain") in Q.SWEEP
    small = large = zero = 0
    for case in Q.SWEEP:
        d = Q.sweep_case(*case)
        t = Q.qr_truth(tau=quantile_midpoints(case[2]).numpy(), gamma=0.99, **d)
        assert int((t["gap"] <= t["gap_bound"]).sum()) <= 0.01 * case[0], case
        rows = np.arange(case[0])
        act = d["action"].astype(np.int64)
        T = d["reward"][:, None].astype(np.float64) + (1 - d["done"][:, None]) * 0.99 * d["target"][rows, t["a_star"]]
        e = T[:, :, None] - d["logit"][rows, act][:, None, :].astype(np.float64)
        small, large, zero = small + int((np.abs(e) < 1).sum()), large + int((np.abs(e) > 1).sum()), zero + int((e == 0).sum())
        if case[3] == "all_done":
            assert d["done"].all()
        if case[3] == "ties":
            assert int((e == 0).sum()) > 0
    assert small > 0 and large > 0 and zero > 0
