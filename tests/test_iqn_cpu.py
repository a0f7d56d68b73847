"""CPU-side checks of the IQN feature: the C ABI carries the new entries, the agent and the mirror network are registered under the
reference's keys, the restatement in tests/iqn_truth.py reproduces the reference's own learn() on the three fixtures
(tools/gen_golden_iqn.py) -- the three forwards, the loss with its statistics, the selected actions, the gradient into the logits and
the parameter gradients at the thinned positions --, the sweep's inputs have the properties the GPU tests rely on, and configuration
errors raise before any GPU use."""
import json
import os
import re

import numpy as np
import pytest
import torch

import iqn_truth as I
from oracle import synth
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["iqn", "iqn_odd", "iqn_cartpole"]
CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, batch=32, num_sample=64, embedding_dim=64, sample_min=0.0, sample_max=1.0,
                    lr=1e-4, eps=1e-2 / 32, gamma=0.99, epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)
NEW_SYMBOLS = ("jh_iqnnet_param_count_for", "jh_iqnnet_create", "jh_iqnnet_destroy", "jh_iqnnet_segment_count", "jh_iqnnet_segment", "jh_iqnnet_set_hyper",
               "jh_iqnnet_set_lr", "jh_iqnnet_sync_target", "jh_iqnnet_forward", "jh_iqnnet_learn_forward", "jh_iqnnet_backward", "jh_iqnnet_optim_step",
               "jh_iqn_cos_features", "jh_iqn_hadamard", "jh_iqn_hadamard_backward", "jh_iqn_loss", "jh_iqn_act")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_iqn_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "iqn.py:" in src  # every declaration cites the reference lines it replaces
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2
    # the layout needs no GPU: widths that are no multiple of 4 and sample counts outside 1..256 have none
    assert lib.jh_iqnnet_param_count_for(4, 512, 64, 64, 2) == 4 * 512 + 512 + 3 * (512 * 512 + 512) + 64 * 512 + 512 + 2 * 512 + 4
    assert lib.jh_iqnnet_param_count_for(4, 30, 64, 64, 2) == -1
    assert lib.jh_iqnnet_param_count_for(4, 32, 16, 0, 2) == -1 and lib.jh_iqnnet_param_count_for(4, 32, 16, 257, 2) == -1


def test_agent_is_registered_under_the_reference_key(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.iqn import IQN

    assert agent_dict["iqn"] is IQN
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("iqn", state_size=4, action_size=2)


UNSUPPORTED = [
    dict(head="cnn", state_size=(4, 84, 84)),
    dict(head="cnn"),
    dict(state_size=(4,)),
    dict(network="discrete_q_network"),
    dict(network="rainbow"),
    dict(optim_config={"name": "rmsprop", "lr": 1e-4}),
    dict(optim_config={"name": "adam", "lr": 1e-4, "weight_decay": 0.1}),
    dict(num_sample=0),
    dict(num_sample=257),
    dict(sample_min=-0.1),
    dict(sample_max=1.5),
    dict(sample_min=0.6, sample_max=0.4),
]


@pytest.mark.parametrize("over", UNSUPPORTED, ids=[",".join(f"{k}={v}" for k, v in o.items()).replace(" ", "")[:48] for o in UNSUPPORTED])
def test_configuration_errors_raise_before_any_gpu_use(over):
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.iqn import IQN_ELIGIBLE

    kw = dict(state_size=4, action_size=2)
    kw.update(over)
    with pytest.raises(ValueError, match="libjorldy_hip") as e:
        Agent("iqn", **kw)
    assert IQN_ELIGIBLE in str(e.value) and "num_sample <= 256" in str(e.value) and "'mlp'" in str(e.value)


def _weights(z, seed_offset):
    shapes = {k[len("shape/"):]: tuple(int(v) for v in z[k]) for k in z.files if k.startswith("shape/")}
    return synth.recipe_state_dict(shapes, int(z["recipe_seed"]) + seed_offset)


def _thin(z, a):
    return synth.thin(a, stride=int(z["thin_stride"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_mirror_network_has_the_fixture_keys_shapes_and_the_reference_initialisation(name):
    from jorldy_amd.core.network import Network

    z = load(name)
    S, A, E, N, H = (int(z[f"hyper/{k}"]) for k in ("S", "A", "E", "N", "H"))
    torch.manual_seed(0)
    net = Network("iqn", S, A, E, N)
    assert H == 512 and net.N_sample == N
    sd = net.state_dict()
    shapes = [(k[len("shape/"):], tuple(int(v) for v in z[k])) for k in z.files if k.startswith("shape/")]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == shapes and tuple(k for k, _ in shapes) == I.KEYS
    # iqn.py:23 names sample_embed twice and state_embed never: orthogonal columns / zero bias there, nn.Linear's default here
    w = sd["sample_embed.weight"].double()
    assert torch.allclose(w.t() @ w, 2.0 * torch.eye(E, dtype=torch.float64), atol=1e-4) and not sd["sample_embed.bias"].any()
    bound = 1.0 / np.sqrt(H)
    assert sd["state_embed.bias"].abs().max() > 0 and sd["state_embed.weight"].abs().max() <= bound and sd["state_embed.bias"].abs().max() <= bound
    for k in ("l1", "l2"):
        w = sd[f"{k}.weight"].double()
        assert torch.allclose(w @ w.t(), 2.0 * torch.eye(H, dtype=torch.float64), atol=1e-3) and not sd[f"{k}.bias"].any()
    w = sd["q.weight"].double()
    assert torch.allclose(w @ w.t(), torch.eye(A, dtype=torch.float64), atol=1e-4)


@pytest.mark.parametrize("name", FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    z = load(name)
    B, N, A, E = (int(z[f"hyper/{k}"]) for k in ("B", "N", "A", "E"))
    gamma = float(z["hyper/gamma"])
    tau = z["learn/tau"]
    assert tau.shape == (3, B, N) and tau.dtype == np.float32 and z["learn/logit"].shape == (B, N, A)
    w0, wt = _weights(z, 0), _weights(z, 1)
    for k in z.files:  # the recipe gives back the weights the reference ran with
        if k.startswith("sd0_thin/"):
            assert np.array_equal(_thin(z, w0[k[9:]]), z[k]) and np.array_equal(_thin(z, wt[k[9:]]), z["sdt_thin/" + k[9:]]), k
    # ---- the loss on the fixture's own logits, in the reference's precision and in float64 (tolerances of test_qrdqn_cpu / test_mdqn_cpu)
    args = (z["learn/logit"], z["learn/logit_next"], z["learn/logit_target"], z["learn/action"], z["learn/reward"], z["learn/done"], tau[0], gamma)
    ref_g = z["learn/d_logit"].astype(np.float64)
    for dtype in (torch.float32, torch.float64):
        t = I.iqn_loss(*args, dtype=dtype)
        np.testing.assert_allclose(t["loss"], float(z["learn/loss"]), rtol=1e-6)
        np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-6)
        err = float(np.abs(t["grad"] - ref_g).max())
        assert err <= 1e-6 * float(np.abs(ref_g).max()), (dtype, err)
        assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(-1).astype(np.int64))
        for k in ("max_Q", "max_logit", "min_logit"):
            np.testing.assert_allclose(t[k], float(z[f"result/{k}"]), rtol=1e-6, err_msg=k)
        assert int((t["gap"] <= t["gap_bound"]).sum()) == 0  # no fixture row has a near-tie of its two best next actions
    act = z["learn/action"].reshape(-1).astype(np.int64)
    np.testing.assert_array_equal(z["learn/theta_pred"].reshape(B, N), z["learn/logit"][np.arange(B), :, act])
    other = np.ones((B, N, A), bool)
    other[np.arange(B), :, act] = False
    assert not ref_g[other].any()
    # ---- the three forwards from the recipe weights, the sampled rows and the recorded draws.  The reference's float32 network stays
    # within 1e-5 of float64 relative to the largest logit (five layers of at most 512-term float32 sums: ~sqrt(512) 2^-24 each)
    x, xn = z["learn/state"], z["learn/next_state"]
    sd64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w0.items()}
    lg = I.iqn_forward(sd64, x, tau[0])
    with torch.no_grad():
        lg_next = I.iqn_forward(w0, xn, tau[1])
        lg_tgt = I.iqn_forward(wt, xn, tau[2])
    for ours, key in ((lg, "logit"), (lg_next, "logit_next"), (lg_tgt, "logit_target")):
        ref = z[f"learn/{key}"].astype(np.float64)
        err = float(np.abs(ours.detach().numpy() - ref).max())
        assert err <= 1e-5 * float(np.abs(ref).max()), (key, err)
    # ---- the whole learn() in float64: loss and the parameter gradients at the thinned positions (1e-5 of the tensor's largest entry)
    t = I.iqn_loss(lg, lg_next, lg_tgt, z["learn/action"], z["learn/reward"], z["learn/done"], tau[0], gamma)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-5)
    assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(-1).astype(np.int64))
    t["loss_t"].backward()
    for k in I.KEYS:
        g = sd64[k].grad.numpy()
        err = float(np.abs(_thin(z, g) - z[f"grad_thin/{k}"]).max())
        assert err <= 1e-5 * float(z[f"grad_absmax/{k}"]), (k, err)
    gn = np.sqrt(sum(float((sd64[k].grad.numpy() ** 2).sum()) for k in I.KEYS))
    np.testing.assert_allclose(gn, float(z["grad_norm"]), rtol=1e-5)


def test_the_cosine_argument_is_the_float32_product():
    """torch forms arange(0, E) * np.pi as float32(i) * float32(pi) and tau * i_pi as a float32 product: the restatement's numpy
    arithmetic gives the same bits, and the float64 product does not (which is why the truth may not use it)."""
    E = 64
    ip = (torch.arange(0, E) * np.pi).numpy()
    assert ip.dtype == np.float32 and np.array_equal(ip.view(np.uint32), I.i_pi(E).view(np.uint32))
    tau = torch.rand(257, generator=torch.Generator().manual_seed(0))
    arg = (tau.view(-1, 1) * torch.from_numpy(ip).view(1, E)).numpy()
    assert np.array_equal(arg.view(np.uint32), I.cos_argument(tau.numpy(), E).view(np.uint32))
    exact = tau.double().view(-1, 1).numpy() * (np.arange(E) * np.pi)
    assert float(np.abs(np.cos(exact) - np.cos(arg.astype(np.float64))).max()) > 1e-6


def test_sweep_covers_the_cases_and_float32_stays_close_to_float64():
    assert I.SWEEP_SHAPES == [(1, 1, 1), (7, 5, 33), (32, 2, 64), (255, 6, 51), (3, 4, 256)] and I.VARIANTS == ("plain", "all_done", "large")
    assert len(I.SWEEP) == 15
    for B, A, N, variant in I.SWEEP:
        d = I.sweep_case(B, A, N, variant)
        t64, t32 = I.iqn_loss(gamma=0.99, **d), I.iqn_loss(gamma=0.99, dtype=torch.float32, **d)
        assert int((t64["gap"] <= t64["gap_bound"]).sum()) <= 0.01 * B, (B, A, N, variant)
        assert float(np.abs(t32["grad"] - t64["grad"]).max()) <= 2e-6 * float(np.abs(t64["grad"]).max()), (B, A, N, variant)
        assert abs(t32["loss"] - t64["loss"]) <= 2e-6 * abs(t64["loss"]), (B, A, N, variant)
        if variant == "all_done":
            assert d["done"].all()
        if variant == "large":
            assert t64["abs_e_min"] > 1.0
        if variant == "plain" and B * N > 1:
            assert t64["abs_e_min"] < 1.0 < t64["abs_e_max"]
    assert I.NET_SHAPES == [(4, 3, 32, 16, 8, 32), (6, 5, 64, 10, 33, 7), (4, 2, 512, 64, 64, 4)]


def test_hadamard_backward_truth_is_the_closed_form():
    rs = np.random.RandomState(0)
    B, N, H = 3, 5, 8
    pp, fp, g = rs.randn(B, H), rs.randn(B, N, H), rs.randn(B, N, H)
    dpsi, dphi = I.hadamard_backward(pp, fp, g)
    psi, phi = np.maximum(pp, 0), np.maximum(fp, 0)
    np.testing.assert_allclose(dphi.numpy(), g * psi[:, None, :] * (fp > 0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(dpsi.numpy(), (g * phi).sum(1) * (pp > 0), rtol=1e-12, atol=1e-15)


def test_curve_fixture_was_made_with_the_config_the_gpu_test_runs():
    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_iqn.json")) as f:
        fx = json.load(f)
    assert fx["iqn_cartpole"]["config"] == CURVE_CONFIG
    ref = fx["iqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == CURVE_CONFIG["steps"] // CURVE_CONFIG["chunk"] for r in ref)
    # the DQN curve test's assertions hold for the reference's own three seeds: the GPU test keeps all three
    start, end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    assert start < 40 and end > 4 * start
