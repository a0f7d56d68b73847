"""CPU-side checks of the Rainbow-IQN feature: the C ABI carries the new entries, the agent and the parameter container are registered under
the reference's keys, the restatement in tests/riqn_truth.py reproduces the reference's own learn() on the three fixtures
(tools/gen_golden_riqn.py) -- the three forwards under the recorded tau and noise draws, theta_target, the per-sample loss, the priorities,
the loss with its statistics, the gradient into the logits and the parameter gradients at the thinned positions --, every ineligible
configuration raises before any GPU use, and no row of the GPU sweep sits where float32 and float64 may legitimately part."""
import os
import re

import numpy as np
import pytest
import torch

import riqn_truth as R
from oracle import synth
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["riqn", "riqn_odd", "riqn_cartpole"]
NEW_SYMBOLS = ("jh_riqnnet_param_count_for", "jh_riqnnet_create", "jh_riqnnet_segment_count", "jh_riqnnet_noise_len", "jh_riqnnet_forward", "jh_riqnnet_learn_forward",
               "jh_riqn_loss")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_riqn_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "rainbow_iqn.py:" in src  # every declaration cites the reference lines it replaces
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    # the layout needs no GPU: trunk (IQN's without q) + (mu, sig) x (a1 | v1 [2H][H] + 2H, a2 [A][H] + A, v2 [H] + 1), every segment padded to 4
    up4 = lambda v: (v + 3) // 4 * 4
    S, H, E, A = 4, 512, 64, 2
    trunk = S * H + H + 3 * (H * H + H) + E * H + H
    tail = 2 * (2 * H * H + 2 * H + up4(A * H) + up4(A) + H + up4(1))
    assert lib.jh_riqnnet_param_count_for(S, H, E, 64, A) == trunk + tail
    assert lib.jh_riqnnet_param_count_for(4, 30, 64, 64, 2) == -1  # hidden_size % 4
    assert lib.jh_riqnnet_param_count_for(2, 32, 64, 64, 2) == -1  # state_size % 4
    assert lib.jh_riqnnet_param_count_for(4, 32, 16, 0, 2) == -1 and lib.jh_riqnnet_param_count_for(4, 32, 16, 257, 2) == -1
    assert lib.jh_riqnnet_segment_count() == 24 and lib.jh_iqnnet_segment_count() == 12


def test_agent_is_registered_under_the_reference_key(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.rainbow import Rainbow
    from jorldy_amd.core.agent.rainbow_iqn import RainbowIQN

    assert agent_dict["rainbow_iqn"] is RainbowIQN and issubclass(RainbowIQN, Rainbow)
    for name in ("process", "interact_callback", "learn", "_idx_offset", "_write_back_priorities", "_draw_noise", "save", "load"):
        assert getattr(RainbowIQN, name) is getattr(Rainbow, name), name  # Rainbow's, unchanged
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("rainbow_iqn", state_size=4, action_size=2)


class _AnyGradSync:
    """A data-parallel hook of any kind.  Its text is part of a test id below, so it carries no memory address."""

    def __repr__(self):
        return "<any>"


UNSUPPORTED = [
    dict(head="cnn", state_size=(4, 84, 84)),  # config.rainbow_iqn.atari / procgen / super_mario_bros
    dict(head="cnn"),
    dict(head="multi"),
    dict(state_size=(4,)),
    dict(state_size=2),  # config.rainbow_iqn.mountaincar
    dict(state_size=6),
    dict(hidden_size=30),
    dict(network="rainbow"),
    dict(network="iqn"),
    dict(noise_type="gaussian"),
    dict(optim_config={"name": "rmsprop", "lr": 1e-4}),
    dict(optim_config={"name": "adam", "lr": 1e-4, "weight_decay": 0.1}),
    dict(num_sample=0),
    dict(num_sample=257),
    dict(action_size=1),
    dict(action_size=65),
    dict(sample_min=0.6, sample_max=0.4),
    dict(frame_dedup=True),
    dict(grad_sync=_AnyGradSync()),
    dict(batch_size=4096, num_sample=256, hidden_size=512),  # 3 * 4096 * 256 * 1024 >= 2^31
]


@pytest.mark.parametrize("over", UNSUPPORTED, ids=[",".join(f"{k}={v}" for k, v in o.items()).replace(" ", "")[:40] for o in UNSUPPORTED])
def test_ineligible_configurations_raise_before_any_gpu_use(over):
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.rainbow_iqn import RIQN_ELIGIBLE

    kw = dict(state_size=4, action_size=2)
    kw.update(over)
    with pytest.raises(ValueError, match="libjorldy_hip") as e:
        Agent("rainbow_iqn", **kw)
    assert RIQN_ELIGIBLE in str(e.value) and "mountaincar" in RIQN_ELIGIBLE and "state_size % 4 == 0" in RIQN_ELIGIBLE


def _weights(z, seed_offset):
    shapes = {k[len("shape/"):]: tuple(int(v) for v in z[k]) for k in z.files if k.startswith("shape/")}
    return synth.recipe_state_dict(shapes, int(z["recipe_seed"]) + seed_offset)


def _thin(z, a):
    return synth.thin(a, limit=int(z["thin_limit"]), stride=int(z["thin_stride"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_parameter_container_has_the_fixture_keys_shapes_and_the_reference_initialisation(name):
    from jorldy_amd.core.network import Network

    z = load(name)
    S, A, E, N, H = (int(z[f"hyper/{k}"]) for k in ("S", "A", "E", "N", "H"))
    noise_type = str(z["hyper/noise_type"])
    torch.manual_seed(0)
    net = Network("rainbow_iqn", S, A, E, N, noise_type, D_hidden=H)
    sd = net.state_dict()
    shapes = [(k[len("shape/"):], tuple(int(v) for v in z[k])) for k in z.files if k.startswith("shape/")]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == shapes and tuple(k for k, _ in shapes) == R.KEYS
    assert [k for k, _ in net.named_parameters()] == list(R.KEYS)  # the optimizer's order
    # rainbow_iqn.py:40 names sample_embed twice and state_embed never
    bound = 1.0 / np.sqrt(H)
    assert not sd["sample_embed.bias"].any() and sd["state_embed.bias"].abs().max() > 0 and sd["state_embed.weight"].abs().max() <= bound
    for k in ("l1", "l2"):
        w = sd[f"{k}.weight"].double()
        assert torch.allclose(w @ w.t(), 2.0 * torch.eye(H, dtype=torch.float64), atol=1e-3) and not sd[f"{k}.bias"].any()
    mu, sig = (1.0 / np.sqrt(H), 0.5 / np.sqrt(H)) if noise_type == "factorized" else (np.sqrt(3.0 / H), 0.017)
    for tag in ("a1", "v1", "a2", "v2"):
        assert sd[f"mu_w_{tag}"].abs().max() <= mu and sd[f"mu_b_{tag}"].abs().max() <= mu
        assert torch.all(sd[f"sig_w_{tag}"] == np.float32(sig)) and torch.all(sd[f"sig_b_{tag}"] == np.float32(sig))


def _loss_args(z, p):
    return (z[p + "logit"], z[p + "logit_next"], z[p + "logit_target"], z[p + "action"], z[p + "reward"], z[p + "done"], z[p + "weights"], z[p + "tau"][0])


@pytest.mark.parametrize("name", FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    z = load(name)
    B, N, A, E, H, n_step = (int(z[f"hyper/{k}"]) for k in ("B", "N", "A", "E", "H", "n_step"))
    gamma, alpha, noise_type = float(z["hyper/gamma"]), float(z["hyper/alpha"]), str(z["hyper/noise_type"])
    w0, wt = _weights(z, 0), _weights(z, 1)
    for k in z.files:  # the recipe gives back the weights the reference ran with
        if k.startswith("sd0_thin/"):
            assert np.array_equal(_thin(z, w0[k[9:]]), z[k]) and np.array_equal(_thin(z, wt[k[9:]]), z["sdt_thin/" + k[9:]]), k
    assert any(k.startswith("sd0_thin/") for k in z.files)
    # ---- the loss on the fixture's own logits, both recorded learns, in the reference's precision and in float64 (test_iqn_cpu's tolerances)
    for p, res in (("learn/", "result/"), ("learn2/", "learn2/result/")):
        tau, noise = z[p + "tau"], z[p + "noise"]
        assert tau.shape == (3, B, N) and tau.dtype == np.float32 and noise.shape == (3, R.noise_len(H, A, noise_type)) and noise.dtype == np.float32
        assert z[p + "logit"].shape == (B, N, A) and z[p + "reward"].shape == (B, n_step, 1) and z[p + "done"].shape == (B, n_step, 1)
        ref_g = z[p + "d_logit"].astype(np.float64)
        for dtype in (torch.float32, torch.float64):
            t = R.riqn_loss(*_loss_args(z, p), gamma, alpha, dtype=dtype)
            np.testing.assert_allclose(t["loss"], float(z[p + "loss"]), rtol=1e-6)
            np.testing.assert_allclose(t["loss"], float(z[res + "loss"]), rtol=1e-6)
            # the reference folds in float32: a product and a sum per step, each rounded by at most half an ulp of the largest |T|
            fold = 2 * n_step * 2.0 ** -24 * float(np.abs(z[p + "theta_target"]).max())
            np.testing.assert_allclose(t["theta_target"], z[p + "theta_target"].reshape(B, N), rtol=0, atol=fold)
            np.testing.assert_allclose(t["loss_b"], z[p + "loss_b"], rtol=1e-6)
            np.testing.assert_allclose(t["prio"], z[p + "p_j"], rtol=1e-6)
            err = float(np.abs(t["grad"] - ref_g).max())
            assert err <= 1e-6 * float(np.abs(ref_g).max()), (dtype, err)
            assert np.array_equal(t["a_star"], z[p + "max_a"].reshape(-1).astype(np.int64))
            for k in ("max_Q", "max_logit", "min_logit"):
                np.testing.assert_allclose(t[k], float(z[res + k]), rtol=1e-6, err_msg=k)
            assert int((t["gap"] <= t["gap_bound"]).sum()) == 0  # no fixture row has a near-tie of its two best next actions
        # the tree the reference left: the priorities at the sampled leaves (the last write wins where a leaf was sampled twice), sums above
        idx = z[p + "indices"].astype(np.int64)
        tp = "" if p == "learn/" else p  # the first learn's tree sits where test_agents_gpu._fill_from_fixture reads it
        tree1 = z[tp + "tree1"]
        last = {int(i): float(v) for i, v in zip(idx, z[p + "p_j"])}
        for i, v in last.items():
            assert tree1[i] == v
        first_leaf = (tree1.size + 1) // 2 - 1
        np.testing.assert_allclose(tree1[0], tree1[first_leaf:].sum(), rtol=1e-12)
        np.testing.assert_allclose(float(z[res + "sampled_p"]), z[tp + "tree0"][idx].mean(), rtol=1e-12)
    if name == "riqn":  # a done at the first, a middle and the last step of a sampled window
        d = z["learn/done"].reshape(B, n_step).astype(bool)
        assert {0, n_step // 2, n_step - 1} <= set(np.argmax(d[d.sum(1) == 1], 1).tolist())
    act = z["learn/action"].reshape(-1).astype(np.int64)
    np.testing.assert_array_equal(z["learn/theta_pred"].reshape(B, N), z["learn/logit"][np.arange(B), :, act])
    # ---- the three forwards of the first learn from the recipe weights, the sampled rows and the recorded draws, at 1e-5 of the largest logit
    x, xn, tau, noise = z["learn/state"], z["learn/next_state"], z["learn/tau"], z["learn/noise"]
    sd64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w0.items()}
    lg = R.riqn_forward(sd64, x, tau[0], noise[0], noise_type)
    with torch.no_grad():
        lg_next = R.riqn_forward(w0, xn, tau[1], noise[1], noise_type)
        lg_tgt = R.riqn_forward(wt, xn, tau[2], noise[2], noise_type)
    for ours, key in ((lg, "logit"), (lg_next, "logit_next"), (lg_tgt, "logit_target")):
        ref = z[f"learn/{key}"].astype(np.float64)
        err = float(np.abs(ours.detach().numpy() - ref).max())
        assert err <= 1e-5 * float(np.abs(ref).max()), (key, err)
    # ---- the whole learn() in float64: loss and the parameter gradients at the thinned positions (1e-5 of the tensor's largest entry)
    t = R.riqn_loss(lg, lg_next, lg_tgt, z["learn/action"], z["learn/reward"], z["learn/done"], z["learn/weights"], tau[0], gamma, alpha)
    np.testing.assert_allclose(t["loss"], float(z["result/loss"]), rtol=1e-5)
    np.testing.assert_allclose(t["loss_b"], z["learn/loss_b"], rtol=1e-5)
    np.testing.assert_allclose(t["prio"], z["learn/p_j"], rtol=1e-5)
    assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(-1).astype(np.int64))
    t["loss_t"].backward()
    for k in R.KEYS:
        g = sd64[k].grad.numpy()
        err = float(np.abs(_thin(z, g) - z[f"grad_thin/{k}"]).max())
        assert err <= 1e-5 * float(z[f"grad_absmax/{k}"]), (k, err)
    gn = np.sqrt(sum(float((sd64[k].grad.numpy() ** 2).sum()) for k in R.KEYS))
    np.testing.assert_allclose(gn, float(z["grad_norm"]), rtol=1e-5)


def test_evaluation_forward_is_the_noise_free_network_and_noise_sets_split_in_draw_order():
    z = load("riqn_odd")
    A, H = int(z["hyper/A"]), int(z["hyper/H"])
    w0 = _weights(z, 0)
    x, tau = z["learn/state"], z["learn/tau"][0]
    plain = R.riqn_forward(w0, x, tau, None)
    zero = R.riqn_forward(w0, x, tau, np.zeros(R.noise_len(H, A, "independent"), np.float32), "independent")
    assert torch.equal(plain, zero)
    d = R.split_noise(z["learn/noise"][0], H, A, "independent")
    assert [tuple(v.shape) for t in ("a1", "v1", "a2", "v2") for v in d[t]] == [(H, H), (H,), (H, H), (H,), (H, A), (A,), (H, 1), (1,)]
    assert np.array_equal(np.concatenate([np.concatenate([d[t][0].reshape(-1), d[t][1]]) for t in ("a1", "v1", "a2", "v2")]), z["learn/noise"][0])
    assert R.noise_len(64, 3, "factorized") == 6 * 64 + 3 + 1


def test_no_row_of_the_gpu_sweep_sits_on_a_near_tie_or_a_kink():
    """The truth alone keeps every row of every case: the selector's two best means are further apart than two float32 sums of N terms can be
    off by, and every |e| is at least 2^-20 (in fact 2^-9, by construction) from 0 and from 1 -- so no case passes a_star."""
    assert R.SWEEP_B == (1, 3, 257) and R.SWEEP_A == (2, 5, 64) and R.SWEEP_N == (1, 63, 64, 65, 256) and R.SWEEP_STEPS == (1, 2, 5) and len(R.SWEEP) == 135
    positions = set()
    for B, A, N, n_step in R.SWEEP:
        d, seed = R.sweep_case(B, A, N, n_step)
        gap, bound = R.selection_gaps(d["next_online"])
        assert (gap > bound).all(), (B, A, N, n_step)
        assert d["reward"].shape == (B, n_step) and 0.1 <= d["weights"].min() and d["weights"].max() == 1.0
        single = d["done"].sum(1) == 1
        positions |= {(n_step, int(p)) for p in np.argmax(d["done"][single], 1)}
        if B * N * N <= 3 * 65 * 65:  # the pairwise errors themselves where they are few ...
            t = R.riqn_loss(gamma=R.SWEEP_GAMMA, alpha=R.SWEEP_ALPHA, **d)
            assert (t["kink"] >= 2.0 ** -9).all() and (t["kink"] > R.KINK).all(), (B, A, N, n_step)
            assert np.array_equal(t["a_star"], np.asarray(d["next_online"], np.float64).mean(1).argmax(-1))
        # ... and the grids they come from everywhere: P on odd multiples of 2^-9, targets and rewards on multiples of 1/4 and 1/2, gamma 1/2
        assert np.array_equal(np.mod(d["logit"].astype(np.float64) * 512, 2), np.ones(d["logit"].shape))
        assert not np.mod(d["target"].astype(np.float64) * 4, 1).any() and not np.mod(d["reward"].astype(np.float64) * 2, 1).any() and R.SWEEP_GAMMA == 0.5
    assert positions >= {(n, p) for n in R.SWEEP_STEPS for p in range(n)}  # a done at every window position


def test_float32_comparator_stays_close_to_float64_on_the_sweep():
    for B, A, N, n_step in [c for c in R.SWEEP if c[0] == 3]:
        d, _ = R.sweep_case(B, A, N, n_step)
        t64 = R.riqn_loss(gamma=R.SWEEP_GAMMA, alpha=R.SWEEP_ALPHA, **d)
        t32 = R.riqn_loss(gamma=R.SWEEP_GAMMA, alpha=R.SWEEP_ALPHA, dtype=torch.float32, **d)
        assert float(np.abs(t32["grad"] - t64["grad"]).max()) <= 2e-6 * float(np.abs(t64["grad"]).max()), (B, A, N, n_step)
        assert abs(t32["loss"] - t64["loss"]) <= 2e-6 * abs(t64["loss"])
        np.testing.assert_allclose(t32["prio"], t64["prio"], rtol=2e-6)


CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, hidden_size=128, batch=32, num_sample=32, embedding_dim=64, sample_min=0.0, sample_max=1.0, lr=1e-4,
                    eps=1e-2 / 32, gamma=0.99, start=2000, target=1000, buffer=50000, lr_decay=True, n_step=3, alpha=0.6, beta=0.4, learn_period=2,
                    uniform_sample_prob=1e-3, noise_type="factorized")


def test_curve_fixture_was_made_with_the_config_the_gpu_test_runs():
    import json

    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_riqn.json")) as f:
        fx = json.load(f)
    assert fx["riqn_cartpole"]["config"] == CURVE_CONFIG
    ref = fx["riqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == CURVE_CONFIG["steps"] // CURVE_CONFIG["chunk"] for r in ref)
    # the IQN curve test's criteria hold for the reference's own three seeds at the reduced agent: the GPU test keeps all three assertions
    start, end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    assert fx["reference_learns"] is True and start < 40 and end > 4 * start
