"""CPU-side checks of the SAC feature: the C ABI carries the new entries, the agent and the policy container are registered under the
reference's keys, the restatement in tests/sac_truth.py reproduces the reference's own learn() on the three fixtures
(tools/gen_golden_sac.py) at half the tolerances the GPU test gives the kernels -- a', logp', y, q, the actor step's a, logp and min_q, every
result key, the parameter gradients and log_alpha after its Adam step, the second of two consecutive learns included --, the mirrors built in
the reference's construction order give the reference's initial weights bit for bit, the case builders have the properties the GPU tests
rely on, and configuration errors raise before any GPU use."""
import json
import os
import re

import numpy as np
import pytest
import torch

import sac_truth as D
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("jh_sac_sample", "jh_sac_critic_loss", "jh_sac_actor_seed", "jh_sac_sample_backward", "jh_sacnet_param_counts_for", "jh_sacnet_create",
               "jh_sacnet_destroy", "jh_sacnet_segment_count", "jh_sacnet_segment", "jh_sacnet_set_hyper", "jh_sacnet_set_lr", "jh_sacnet_set_alpha", "jh_sacnet_get_alpha",
               "jh_sacnet_sync_target", "jh_sacnet_soft_update", "jh_sacnet_actor_forward", "jh_sacnet_critic_forward", "jh_sacnet_critic_update", "jh_sacnet_actor_update")
CURVE_CONFIG = D.CURVE_CONFIG


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_table_carry_the_new_entries(lib):
    import ctypes as C

    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "sac.py:" in src and "policy.py:38-55" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2
    assert lib.jh_acnet_segment_count() == 14 and lib.jh_sacnet_segment_count() == 16
    # the layout needs no GPU
    na, nc = C.c_int64(), C.c_int64()
    assert lib.jh_sacnet_param_counts_for(11, 512, 3, C.byref(na), C.byref(nc)) == 0
    assert na.value == 11 * 512 + 512 + 512 * 512 + 512 + 2 * 3 * 512 + 8  # mu and log_std as one [2A][H] layer, its [2A] bias padded to 8
    assert nc.value == 11 * 512 + 512 + 3 * 512 + 512 + 1024 * 512 + 512 + 512 + 4
    assert lib.jh_sacnet_param_counts_for(11, 30, 3, C.byref(na), C.byref(nc)) != 0 and b"bad argument" in lib.jh_last_error()
    assert lib.jh_sacnet_param_counts_for(11, 32, 0, C.byref(na), C.byref(nc)) != 0


def test_agent_and_policy_are_registered_under_the_reference_keys(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.sac import SAC
    from jorldy_amd.core.network import ContinuousPolicy, network_dict

    assert agent_dict["sac"] is SAC and SAC.action_type == "continuous"
    assert network_dict["continuous_policy"] is ContinuousPolicy
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("sac", state_size=4, action_size=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("sac", state_size=4, action_size=2, use_dynamic_alpha=True, target_update_period=7, some_unknown_keyword=1)


@pytest.mark.parametrize("name", D.FIXTURES)
def test_mirror_networks_have_the_fixture_keys_and_shapes(name):
    from jorldy_amd.core.network import Network

    z = load(name)
    fx = D.Fixture(z)
    actor = Network("continuous_policy", fx.S, fx.A, D_hidden=fx.H, head="mlp")
    critic = Network("continuous_q_network", fx.S, fx.A, D_hidden=fx.H, head="mlp")
    assert fx.nets == ("actor", "critic1", "target_critic1", "critic2", "target_critic2")
    for net in fx.nets:
        sd = (actor if net == "actor" else critic).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in D.shapes_of(net, fx.S, fx.A, fx.H).items()], net
        stored = [k[len(f"sd0/{net}/"):] for k in z.files if k.startswith(f"sd0/{net}/")]
        assert stored == list(sd.keys()), net
    assert tuple(actor.state_dict().keys()) == D.ACTOR_KEYS == ("head.l.weight", "head.l.bias", "l.weight", "l.bias", "mu.weight", "mu.bias", "log_std.weight", "log_std.bias")
    # the truth's forward-capable mirrors carry the same keys
    assert list(D.Actor(fx.S, fx.A, fx.H).state_dict().keys()) == list(actor.state_dict().keys())
    assert list(D.Critic(fx.S, fx.A, fx.H).state_dict().keys()) == list(critic.state_dict().keys())


@pytest.mark.parametrize("name", D.FIXTURES)
def test_mirrors_in_the_reference_construction_order_give_the_reference_initial_weights(name):
    """sac.py:75-95: actor, critic 1, its target, critic 2, its target.  Every module draws from torch's generator when it is built, the targets
    too, before they are overwritten: under the recorded seed the ONLINE networks must come out bit for bit as the reference's (the stored
    targets equal their online nets).  One torch thread, as the generator ran: orthogonal_ goes through a QR factorisation whose blocked
    products round differently with the thread count."""
    from oracle import synth

    from jorldy_amd.core.network import Network

    z = load(name)
    fx = D.Fixture(z)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.manual_seed(int(z["hyper/init_seed"]))
        built = {}
        for net in fx.nets:
            built[net] = Network("continuous_policy" if net == "actor" else "continuous_q_network", fx.S, fx.A, D_hidden=fx.H, head="mlp").state_dict()
    finally:
        torch.set_num_threads(threads)
    for net in fx.nets:
        src = built[net.replace("target_", "")]
        for k, v in src.items():
            assert np.array_equal(synth.thin(v.numpy()), z[f"init_thin/{net}/{k}"]), (net, k)
    # orthogonal_init's gains: mu "linear" (1), log_std "tanh" (5/3), every hidden layer "relu" (sqrt 2); biases zero
    eye = torch.eye(fx.A, dtype=torch.float64)
    w = built["actor"]["mu.weight"].double()
    assert torch.allclose(w @ w.t(), eye, atol=1e-4)
    w = built["actor"]["log_std.weight"].double()
    assert torch.allclose(w @ w.t(), (5.0 / 3.0) ** 2 * eye, atol=1e-4)
    w = built["actor"]["l.weight"].double()
    assert torch.allclose(w @ w.t(), 2.0 * torch.eye(fx.H, dtype=torch.float64), atol=1e-3) and not built["actor"]["mu.bias"].any() and not built["actor"]["log_std.bias"].any()


def _half(err, tol, what):
    assert err <= 0.5 * tol, f"{what}: {err:.3e} is more than half of the GPU test's tolerance {tol:.3e}"


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    """Float64 against the reference's float32 run at the GPU test's tolerances, each achieved value at no more than half of its tolerance:
    result keys rtol 1e-5, y / q / a / logp rtol and atol 1e-5, gradients 1e-5 of the tensor's largest entry, log_alpha after its step by
    fp64_truth's per-element criterion."""
    z = load(name)
    fx = D.Fixture(z)
    gamma, te = float(z["hyper/gamma"]), float(z["hyper/target_entropy"])
    assert te == -fx.A and fx.records == (["r0", "r1"] if name == "sac" else ["r0"])
    assert fx.dynamic == (name != "sac_odd")
    for r in fx.records:
        b, eps, sd, al0, al1 = fx.batch(r), fx.eps(r), fx.start(r), fx.alpha(r, 0), fx.alpha(r, 1)
        assert b["state"].shape == (fx.B, fx.S) and b["action"].shape == (fx.B, fx.A) and eps.shape == (2, fx.B, fx.A)
        crit, targ = ["critic1", "critic2"], ["target_critic1", "target_critic2"]
        t = D.critic_update(sd["actor"], [sd[n] for n in crit], [sd[n] for n in targ], b["state"], b["action"], b["reward"], b["next_state"], b["done"], eps[0],
                            gamma, al0["alpha"])

        def close(ours, ref, what):
            ref = np.asarray(ref, dtype=np.float64)
            err = np.abs(np.asarray(ours, dtype=np.float64).reshape(ref.shape) - ref)
            worst = float((err / (1e-5 + 1e-5 * np.abs(ref))).max())
            assert worst <= 0.5, (r, what, worst)

        def scalar(ours, key):
            ref = float(z[f"{r}/result/{key}"])
            _half(abs(float(ours) - ref), 1e-5 * abs(ref), f"{r} {key}")

        close(t["next_action"], z[f"{r}/learn/next_action"], "next_action")
        close(t["logp_next"], z[f"{r}/learn/next_log_prob"], "next_log_prob")
        close(t["y"], z[f"{r}/learn/target_q"], "y")
        close(t["q"][0], z[f"{r}/learn/q1"], "q1")
        close(t["q"][1], z[f"{r}/learn/q2"], "q2")
        scalar(t["max_Q"], "max_Q")
        scalar(t["loss"][0], "critic_loss1")
        scalar(t["loss"][1], "critic_loss2")
        for net, g in zip(crit, t["grads"]):
            for k, v in g.items():
                err = float(np.abs(fx.thin(v.numpy()) - z[f"{r}/grad/{net}/{k}"]).max())
                _half(err, 1e-5 * float(z[f"{r}/grad_absmax/{net}/{k}"]), f"{r} grad {net} {k}")
        # the actor step uses the critics AFTER their step: the truth takes that Adam step itself, in float64, from the gradients it has just
        # computed -- the first step of a fresh optimizer, or (r1 of sac.npz, stored in full) the second one from r0's moments
        lr, first = float(z["hyper/critic_lr"]), r == "r0"
        stepped = []
        for i, net in enumerate(crit):
            m, v = (None, None) if first else fx.moments("r0", net)
            sd_c = D.adam_step(sd[net], t["grads"][i], lr, m, v, 0 if first else 1)
            # ... and lands on the reference's stepped critic within the caps of the agent tests: an Adam step is lr * m / (sqrt(v) + eps), so
            # a float32 gradient next to zero may move a weight by up to 2 lr differently; at most 0.5 % of the weights further than 2e-5
            diff = np.concatenate([np.abs(fx.thin(val.numpy()).astype(np.float64) - z[f"{r}/sd1/{net}/{k}"]).reshape(-1) for k, val in sd_c.items()])
            assert diff.max() <= 2.1 * lr and (diff > 2e-5).mean() <= 0.005, (r, net, diff.max(), (diff > 2e-5).mean())
            stepped.append(sd_c)
        a = D.actor_update(sd["actor"], stepped, b["state"], eps[1], al0["alpha"], al0["log_alpha"], te)
        close(a["action"], z[f"{r}/learn/sample_action"], "sample_action")
        close(a["logp"], z[f"{r}/learn/log_prob"], "log_prob")
        close(a["min_q"], z[f"{r}/learn/min_q"], "min_q")
        for key in ("actor_loss", "alpha_loss", "mean_Q", "entropy"):
            scalar(a[key], key)
        _half(abs(float(a["actor_loss"]) - float(z[f"{r}/learn/actor_loss"])), 1e-5 * abs(float(z[f"{r}/learn/actor_loss"])), "actor_loss at the tap")
        for k, v in a["grads"].items():
            err = float(np.abs(fx.thin(v.numpy()) - z[f"{r}/grad/actor/{k}"]).max())
            _half(err, 1e-5 * float(z[f"{r}/grad_absmax/actor/{k}"]), f"{r} grad actor {k}")
        # the temperature: result["alpha"] is exp(log_alpha BEFORE the step); dynamic: one Adam step of log_alpha; static: nothing moves
        scalar(np.exp(al0["log_alpha"]), "alpha")
        assert al1["alpha"] == float(z[f"{r}/result/alpha"])
        if fx.dynamic:
            alr = float(z["hyper/alpha_lr"])
            w, m, v = D.alpha_adam_step(al0["log_alpha"], float(a["alpha_grad"]), al0["exp_avg"], al0["exp_avg_sq"], al0["step"], alr)
            _half(abs(w - al1["log_alpha"]), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - al0["log_alpha"]) + 1e-6 * alr, f"{r} log_alpha after its step")
            assert al1["step"] == al0["step"] + 1
        else:
            assert al1 == al0 and al0["log_alpha"] == float(z["hyper/static_log_alpha"]) and al0["step"] == 0
        # learn() by itself moves no target
        assert all(int(z[f"{r}/unchanged/{n}"]) for n in targ) and not any(int(z[f"{r}/unchanged/{n}"]) for n in ("actor", "critic1", "critic2"))
    if name == "sac":
        # the one-step lag: r0 and r1 both form their losses with the initial alpha; r1 reports exp(log_alpha after ONE step), which differs visibly
        assert fx.alpha("r0", 0)["alpha"] == 1.0 and fx.alpha("r1", 0)["alpha"] == 1.0 and fx.alpha("r1", 0)["log_alpha"] != 0.0
        assert abs(float(z["r1/result/alpha"]) - 1.0) > 0.04


def test_case_builders_have_the_properties_the_gpu_tests_rely_on():
    assert D.SAMPLE_SHAPES == ((1, 1), (7, 3), (128, 6), (257, 2), (1025, 17)) and D.SPREADS == (0.5, 1.5) and D.LOSS_B == (1, 7, 256, 257, 1025)
    for B, A in D.SAMPLE_SHAPES:
        for s in D.SPREADS:
            mu, ls, eps = D.sample_case(B, A, s)
            assert mu.dtype == ls.dtype == eps.dtype == np.float32 and mu.shape == (B, A)
            assert (mu.reshape(-1)[0], ls.reshape(-1)[0], eps.reshape(-1)[0]) == (7.0, 0.0, -3.0)
            if B * A > 1:
                assert (mu.reshape(-1)[1], eps.reshape(-1)[1]) == (-5.0, 3.5)
            a64, lp64 = D.sample(mu, ls, eps)
            a32, lp32 = D.sample(mu, ls, eps, torch.float32)
            # the reference's own float32 evaluation stays within K = 1 of the bound the kernel gets K = 4 of
            k_ref = float((np.abs(lp32.double().numpy() - lp64.numpy()) / D.logp_bound(eps, a64.numpy(), 1.0)).max())
            assert k_ref <= 1.0, (B, A, s, k_ref)
            # the backward test's conditions: at most 30 % of the elements are left out of the tight check, and for B >= 128 at the wide spread
            # at least 5 CLAMPED elements stay in it
            well = (1 - a64.numpy() ** 2) >= D.WELL
            assert 1 - well.mean() <= 0.30, (B, A, s, 1 - well.mean())
            assert well.reshape(-1)[0], "the planted clamped element is well conditioned"
            if B >= 128 and s == 1.5:
                assert int(((np.abs(mu) > 5) & well).sum()) >= 5, (B, A)
            g = D.sample_backward(D.sample_da(B, A), mu, ls, eps, D.ALPHA)
            assert float(g[0].reshape(-1)[0]) == 0.0 and (B * A == 1 or float(g[0].reshape(-1)[1]) != 0.0)
    for B in D.LOSS_B:
        for variant in D.LOSS_VARIANTS:
            q, qn, lp, lpn, r, d = D.loss_case(B, variant)
            assert q.shape == (2, B) and qn.shape == (2, B) and lp.shape == (B,)
            if variant == "all_done":
                assert d.all()
                np.testing.assert_array_equal(D.critic_loss(q, qn, lpn, r, d, 0.99, 0.37)["y"].numpy(), r.astype(np.float64))
            if variant == "equal_q":
                assert np.array_equal(q[0], q[1]) and np.array_equal(qn[0], qn[1])
                assert np.array_equal(D.actor_seed(q, lp, 0.37, -0.8, -3.0)["grad"].numpy(), np.full((2, B), -0.5 / B))
            else:
                assert not (q[0] == q[1]).any()


@pytest.mark.parametrize("S,A,H,B", D.NET_SHAPES)
def test_network_case_keeps_the_samples_away_from_saturation(S, A, H, B):
    """The network test's inputs are scaled so that max |z| <= 4 in the truth: saturation is the elementwise tests' ground."""
    actor = D.mirrors(D.Actor, S, A, H, 0)[0]
    _, _, critic, act = D.net_inputs(S, A, B, 3)
    with torch.no_grad():
        for x, eps in [(c["x_all"][B:], c["eps"]) for c in critic] + [(a["x"], a["eps"]) for a in act]:
            mu, std = actor(x.double())
            assert float((mu + std * eps.double()).abs().max()) <= 4.0


def test_curve_fixture_was_made_with_the_config_the_gpu_test_runs():
    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_sac.json")) as f:
        fx = json.load(f)
    assert fx["config"] == CURVE_CONFIG and fx["seeds"] == [1, 2, 3]
    ref = fx["sac"]["reference"]
    assert len(ref) == 3 and all(len(r) == CURVE_CONFIG["steps"] // CURVE_CONFIG["chunk"] for r in ref)
    start, end = np.mean([x[0] for x in ref]), np.mean([np.mean(x[-3:]) for x in ref])
    assert end > start + 0.3, (start, end)  # the GPU test's assertion holds for the reference's own three seeds


UNSUPPORTED = [
    dict(head="cnn", state_size=(4, 84, 84)),
    dict(head="cnn"),
    dict(head="multi"),
    dict(state_size=(4,)),
    dict(hidden_size=30),
    dict(actor="discrete_policy"),
    dict(critic="discrete_q_network"),
    dict(actor="discrete_policy", critic="discrete_q_network"),
    dict(actor="deterministic_policy"),
    dict(optim_config={"actor": "rmsprop", "critic": "adam", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}),
    dict(optim_config={"actor": "adam", "critic": "sgd", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}),
    dict(optim_config={"actor": "adam", "critic": "adam", "alpha": "sgd", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}),
    dict(optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4, "weight_decay": 0.1}),
]


def test_configuration_errors_raise_before_any_gpu_use():
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.sac import SAC_ELIGIBLE

    for over in UNSUPPORTED:
        kw = dict(state_size=4, action_size=2)
        kw.update(over)
        with pytest.raises(ValueError, match="libjorldy_hip") as e:
            Agent("sac", **kw)
        assert SAC_ELIGIBLE in str(e.value)
