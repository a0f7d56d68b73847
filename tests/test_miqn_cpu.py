"""CPU-side checks of the M-IQN feature: the C ABI carries the new entries, the agent is registered under the reference's key,
configuration errors raise before any GPU use, the restatement in tests/miqn_truth.py reproduces the reference's own learn() on the three
fixtures (tools/gen_golden_miqn.py) -- the three forwards the native path keeps, theta_target, the log-policy, the loss with its
statistics (max_logit / min_logit from the FOURTH forward), the gradient into the first forward's logits and the parameter gradients at
the thinned positions --, and the sweep's inputs have the properties the GPU tests rely on."""
import os
import re

import numpy as np
import pytest
import torch

import miqn_truth as M
from oracle import synth
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["miqn", "miqn_odd", "miqn_cartpole"]
MAX_BYTES = 461784  # the family's cap (tools/gen_golden_iqn.py)
NATIVE_SLOTS = [0, 3, 2]  # the reference's draws (online(s), online(s'), target(s'), online(s) again) in the native slot order


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_miqn_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "m_iqn.py:" in src  # every declaration cites the reference lines it replaces
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("jh_miqn_loss", "jh_iqnnet_learn_forward_m"):
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2


def test_agent_is_registered_under_the_reference_key(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.iqn import IQN
    from jorldy_amd.core.agent.miqn import MIQN

    assert agent_dict["m_iqn"] is MIQN and issubclass(MIQN, IQN)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("m_iqn", state_size=4, action_size=2)


UNSUPPORTED = [
    (dict(tau=0), "tau=0"),
    (dict(tau=-0.03), "tau=-0.03"),
    (dict(l_0=0.5), "l_0=0.5"),
    # IQN's own ineligible cases, with IQN's message
    (dict(head="cnn", state_size=(4, 84, 84)), "'cnn'"),
    (dict(state_size=(4,)), None),
    (dict(network="discrete_q_network"), None),
    (dict(optim_config={"name": "rmsprop", "lr": 1e-4}), None),
    (dict(num_sample=0), None),
    (dict(num_sample=257), None),
    (dict(sample_min=0.6, sample_max=0.4), None),
]


@pytest.mark.parametrize("over,needle", UNSUPPORTED, ids=[",".join(f"{k}={v}" for k, v in o.items()).replace(" ", "")[:48] for o, _ in UNSUPPORTED])
def test_configuration_errors_raise_before_any_gpu_use(over, needle):
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.iqn import IQN_ELIGIBLE

    kw = dict(state_size=4, action_size=2)
    kw.update(over)
    with pytest.raises(ValueError, match="libjorldy_hip") as e:
        Agent("m_iqn", **kw)
    assert IQN_ELIGIBLE in str(e.value) and "not on the native engine yet" in str(e.value)
    if needle:
        assert needle in str(e.value)


def _weights(z, seed_offset):
    shapes = {k[len("shape/"):]: tuple(int(v) for v in z[k]) for k in z.files if k.startswith("shape/")}
    return synth.recipe_state_dict(shapes, int(z["recipe_seed"]) + seed_offset)


def _thin(z, a):
    return synth.thin(a, stride=int(z["thin_stride"]))


def _hyper(z):
    return dict(gamma=float(z["hyper/gamma"]), alpha=float(z["hyper/alpha"]), tau_e=float(z["hyper/m_tau"]), l_0=float(z["hyper/l_0"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_holds_what_the_tests_need_within_the_family_cap(name):
    z = load(name)
    B, N, A = (int(z[f"hyper/{k}"]) for k in ("B", "N", "A"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= MAX_BYTES
    assert (float(z["hyper/alpha"]), float(z["hyper/m_tau"]), float(z["hyper/l_0"])) == (0.9, 0.03, -1.0)
    tau = z["learn/tau"]
    assert tau.shape == (4, B, N) and tau.dtype == np.float32 and len({tau[i].tobytes() for i in range(4)}) == 4  # four draws, all different
    for k in ("logit", "logit_again", "logit_target", "d_logit"):
        assert z[f"learn/{k}"].shape == (B, N, A), k
    assert z["learn/theta_target"].shape == (B, N, 1) and z["learn/log_policy"].shape == (B, 1)
    assert set(k[7:] for k in z.files if k.startswith("result/")) == {"loss", "epsilon", "max_Q", "max_logit", "min_logit"}
    # the detail the statistics hang on: max / min logit are the FOURTH forward's, max_Q the first's -- and the fixture can tell them apart
    first, again = z["learn/logit"], z["learn/logit_again"]
    assert float(z["result/max_logit"]) == float(again.max()) != float(first.max())
    assert float(z["result/min_logit"]) == float(again.min()) != float(first.min())
    np.testing.assert_allclose(float(z["result/max_Q"]), first.astype(np.float64).mean(1).max(), rtol=1e-6)
    assert abs(float(z["result/max_Q"]) - again.astype(np.float64).mean(1).max()) > 1e-4 * abs(float(z["result/max_Q"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_float32_truth_reproduces_the_reference_fixture(name):
    """Same operations in the same precision as the reference's learn(): 1e-6, the tolerance of the M-DQN and IQN CPU tests."""
    z = load(name)
    B, N, A = (int(z[f"hyper/{k}"]) for k in ("B", "N", "A"))
    args = (z["learn/logit"], z["learn/logit_again"], z["learn/logit_target"], z["learn/action"], z["learn/reward"], z["learn/done"], z["learn/tau"][0])
    t = M.miqn_loss(*args, dtype=torch.float32, **_hyper(z))
    ref_T = z["learn/theta_target"].reshape(B, N)
    assert float(np.abs(t["theta_target"] - ref_T).max()) <= 1e-6 * float(np.abs(ref_T).max())
    np.testing.assert_allclose(t["log_policy"], z["learn/log_policy"].reshape(-1), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(t["loss"], float(z["learn/loss"]), rtol=1e-6)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-6)
    for k in ("max_Q", "max_logit", "min_logit"):
        np.testing.assert_allclose(t[k], float(z[f"result/{k}"]), rtol=1e-6, err_msg=k)
    ref_g = z["learn/d_logit"]
    assert float(np.abs(t["grad"] - ref_g).max()) <= 1e-6 * float(np.abs(ref_g).max())
    # the reference's own intermediates
    act = z["learn/action"].reshape(-1).astype(np.int64)
    np.testing.assert_array_equal(z["learn/theta_pred"].reshape(B, N), z["learn/logit"][np.arange(B), :, act])
    other = np.ones((B, N, A), bool)
    other[np.arange(B), :, act] = False
    assert not ref_g[other].any()
    lp = z["learn/log_policy"].reshape(-1)
    np.testing.assert_array_equal(z["learn/munchausen_term"].reshape(-1), (np.float32(0.9) * np.clip(lp, -1, 0)).astype(np.float32))
    assert np.array_equal(t["clipped"], lp < -1.0)


@pytest.mark.parametrize("name", FIXTURES)
def test_float64_truth_and_network_reproduce_the_reference_fixture(name):
    z = load(name)
    B, N, A = (int(z[f"hyper/{k}"]) for k in ("B", "N", "A"))
    hy = _hyper(z)
    tau = z["learn/tau"][NATIVE_SLOTS]
    w0, wt = _weights(z, 0), _weights(z, 1)
    for k in z.files:  # the recipe gives back the weights the reference ran with
        if k.startswith("sd0_thin/"):
            assert np.array_equal(_thin(z, w0[k[9:]]), z[k]) and np.array_equal(_thin(z, wt[k[9:]]), z["sdt_thin/" + k[9:]]), k
    # ---- float64 on the fixture's own logits.  The policies divide the quantile means by tau_e = 0.03: the float32 rounding of a mean
    # (<= 2^-24 sqrt(N) |x|, |x| <= 4.7 here) moves a policy weight by up to 33 times that, ~1.5e-5 at N = 64, and theta_target with it:
    # 2e-5 of the largest entry for theta_target and the gradient; the loss averages B N^2 pairs and keeps 1e-6.
    args = (z["learn/logit"], z["learn/logit_again"], z["learn/logit_target"], z["learn/action"], z["learn/reward"], z["learn/done"], tau[0])
    t = M.miqn_loss(*args, **hy)
    ref_T, ref_g = z["learn/theta_target"].reshape(B, N).astype(np.float64), z["learn/d_logit"].astype(np.float64)
    assert float(np.abs(t["theta_target"] - ref_T).max()) <= 2e-5 * float(np.abs(ref_T).max())
    assert float(np.abs(t["grad"] - ref_g).max()) <= 2e-5 * float(np.abs(ref_g).max())
    np.testing.assert_allclose(t["log_policy"], z["learn/log_policy"].reshape(-1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-6)
    for k in ("max_Q", "max_logit", "min_logit"):
        np.testing.assert_allclose(t[k], float(z[f"result/{k}"]), rtol=1e-6, err_msg=k)
    # ---- the three forwards the native path keeps, from the recipe weights, the sampled rows and the recorded draws (IQN's 1e-5)
    x, xn = z["learn/state"], z["learn/next_state"]
    sd64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w0.items()}
    lg = M.iqn_forward(sd64, x, tau[0])
    with torch.no_grad():
        lg_again = M.iqn_forward(w0, x, tau[1])
        lg_tgt = M.iqn_forward(wt, xn, tau[2])
    for ours, key in ((lg, "logit"), (lg_again, "logit_again"), (lg_tgt, "logit_target")):
        ref = z[f"learn/{key}"].astype(np.float64)
        err = float(np.abs(ours.detach().numpy() - ref).max())
        assert err <= 1e-5 * float(np.abs(ref).max()), (key, err)
    # ---- the whole learn() in float64: loss and the parameter gradients at the thinned positions.  The policies see the float32
    # network's error in the means (1e-5 of the largest logit) times 1 / tau_e: 3e-4 for the gradients, which are linear in the
    # clipped errors; the loss keeps 1e-4
    t = M.miqn_loss(lg, lg_again, lg_tgt, z["learn/action"], z["learn/reward"], z["learn/done"], tau[0], **hy)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-4)
    t["loss_t"].backward()
    for k in M.KEYS:
        g = sd64[k].grad.numpy()
        err = float(np.abs(_thin(z, g) - z[f"grad_thin/{k}"]).max())
        assert err <= 3e-4 * float(z[f"grad_absmax/{k}"]), (k, err)


def test_sweep_covers_the_cases_and_float32_stays_close_to_float64():
    assert M.SWEEP_SHAPES == [(1, 1, 1), (7, 5, 33), (32, 2, 64), (255, 6, 51), (3, 4, 256)]
    assert M.VARIANTS == ("plain", "all_done", "large", "wide", "flat", "tau1") and len(M.SWEEP) == 30
    assert M.HYPER == dict(gamma=0.99, alpha=0.9, tau_e=0.03, l_0=-1.0)
    both = []
    for B, A, N, variant in M.SWEEP:
        d, hy = M.sweep_case(B, A, N, variant)
        t64, t32 = M.miqn_loss(**d, **hy), M.miqn_loss(dtype=torch.float32, **d, **hy)
        # float32 against float64: 2e-6 as in IQN's sweep; `wide` (|x| <= 100, 1 / tau_e = 33) amplifies the rounding of a quantile mean
        # (2^-24 sqrt(N) |x|) into a policy weight by 33: 2e-5
        tol = 2e-5 if variant == "wide" else 2e-6
        assert float(np.abs(t32["grad"] - t64["grad"]).max()) <= tol * float(np.abs(t64["grad"]).max()), (B, A, N, variant)
        assert abs(t32["loss"] - t64["loss"]) <= 2e-6 * abs(t64["loss"]), (B, A, N, variant)
        n_clip = int(t64["clipped"].sum())
        assert (hy["tau_e"] == 1.0) == (variant == "tau1")
        if variant == "all_done":
            assert d["done"].all()
        if variant == "large":
            assert t64["abs_e_min"] > 1.0
        if variant == "flat":
            assert n_clip == 0 and float(np.abs(t64["log_policy"]).max()) < 0.1
        if variant == "wide" and A > 1:
            assert n_clip >= 0.4 * B  # one-hot policies: every row whose action is not the best one clips
            x = d["logit_again"].astype(np.float64).mean(1)
            assert np.exp(-(x.max(-1) - x.min(-1)) / hy["tau_e"]).min() == 0.0  # exp underflows, in float64 too
        if A == 1:
            assert not t64["log_policy"].any() and n_clip == 0  # log-policy 0, pi = 1
        if variant == "plain" and 0 < n_clip < B and t64["abs_e_min"] < 1.0 < t64["abs_e_max"]:
            both.append((B, A, N))
    assert both == M.BOTH_SIDES and len(both) >= 3
    assert M.NET_SHAPES == [(4, 3, 32, 16, 8, 32), (6, 5, 64, 10, 33, 7), (4, 2, 512, 64, 64, 4)]
