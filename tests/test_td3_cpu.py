"""CPU-side checks of the TD3 / DDPG feature: the C ABI carries the new entries, the agents and the mirror networks are registered under
the reference's keys, the restatement in tests/td3_truth.py reproduces the reference's own learn() on the five fixtures
(tools/gen_golden_td3.py) -- y, q, losses, max_Q, actor(s), actor_loss and the parameter gradients --, the mirrors built in the
reference's construction order give the reference's initial weights bit for bit, the sweep's inputs have the properties the GPU tests
rely on, and configuration errors raise before any GPU use."""
import json
import os
import re

import numpy as np
import pytest
import torch

import td3_truth as D
from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("jh_td3_next_action", "jh_td3_critic_loss", "jh_td3_actor_seed", "jh_td3_tanh_backward", "jh_td3_polyak", "jh_acnet_param_counts_for",
               "jh_acnet_create", "jh_acnet_destroy", "jh_acnet_segment_count", "jh_acnet_segment", "jh_acnet_set_hyper", "jh_acnet_set_lr", "jh_acnet_sync_target",
               "jh_acnet_soft_update", "jh_acnet_actor_forward", "jh_acnet_critic_forward", "jh_acnet_critic_update", "jh_acnet_actor_update")
CURVE_CONFIG = dict(S=11, A=3, steps=8000, chunk=1000, run_step=10000, hidden=256, batch=128, buffer=50000, start=1000, tau=5e-3, gamma=0.99, lr_decay=True,
                    td3=dict(initial_random_step=1000, actor_lr=1e-3, critic_lr=1e-3), ddpg=dict())


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
    assert "td3.py:" in src and "ddpg.py:" in src and "q_network.py:23-39" in src and "policy.py:8-20" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2
    # the layout needs no GPU
    na, nc = C.c_int64(), C.c_int64()
    assert lib.jh_acnet_param_counts_for(11, 512, 3, C.byref(na), C.byref(nc)) == 0
    assert na.value == 11 * 512 + 512 + 512 * 512 + 512 + 3 * 512 + 4
    assert nc.value == 11 * 512 + 512 + 3 * 512 + 512 + 1024 * 512 + 512 + 512 + 4
    assert lib.jh_acnet_param_counts_for(11, 30, 3, C.byref(na), C.byref(nc)) != 0 and b"bad argument" in lib.jh_last_error()
    assert lib.jh_acnet_param_counts_for(11, 32, 0, C.byref(na), C.byref(nc)) != 0


def test_agents_and_networks_are_registered_under_the_reference_keys(lib):
    from jorldy_amd.core.agent import Agent, agent_dict
    from jorldy_amd.core.agent.ddpg import DDPG
    from jorldy_amd.core.agent.td3 import TD3
    from jorldy_amd.core.network import ContinuousQ_Network, DeterministicPolicy, network_dict

    assert agent_dict["td3"] is TD3 and agent_dict["ddpg"] is DDPG
    assert TD3.action_type == "continuous" and DDPG.action_type == "continuous"
    assert network_dict["deterministic_policy"] is DeterministicPolicy and network_dict["continuous_q_network"] is ContinuousQ_Network
    if not torch.cuda.is_available():
        for name in ("td3", "ddpg"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                Agent(name, state_size=4, action_size=2)


@pytest.mark.parametrize("name", D.FIXTURES)
def test_mirror_networks_have_the_fixture_keys_and_shapes(name):
    from jorldy_amd.core.network import Network

    z = load(name)
    fx = D.Fixture(z)
    actor = Network("deterministic_policy", fx.S, fx.A, D_hidden=fx.H, head="mlp")
    critic = Network("continuous_q_network", fx.S, fx.A, D_hidden=fx.H, head="mlp")
    for net in fx.nets:
        sd = (actor if "actor" in net else critic).state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s in D.shapes_of(net, fx.S, fx.A, fx.H).items()], net
        stored = [k[len(f"sd0/{net}/"):] for k in z.files if k.startswith(f"sd0/{net}/")]
        assert stored == list(sd.keys()), net
    # the truth's forward-capable mirrors carry the same keys
    assert list(D.Actor(fx.S, fx.A, fx.H).state_dict().keys()) == list(actor.state_dict().keys())
    assert list(D.Critic(fx.S, fx.A, fx.H).state_dict().keys()) == list(critic.state_dict().keys())


@pytest.mark.parametrize("name", D.FIXTURES)
def test_mirrors_in_the_reference_construction_order_give_the_reference_initial_weights(name):
    """td3.py:77-112: actor, target actor, critic 1, its target, critic 2, its target; ddpg.py:74-87: actor, critic, target actor, target
    critic.  Every module draws from torch's generator when it is built, the targets too, before they are overwritten: under the recorded
    seed the ONLINE networks must come out bit for bit as the reference's (the stored targets equal their online nets).  One torch thread, as
    the generator ran: orthogonal_ goes through a QR factorisation whose blocked products round differently with the thread count."""
    from oracle import synth

    from jorldy_amd.core.network import Network

    z = load(name)
    fx = D.Fixture(z)
    order = fx.nets if fx.kind == "td3" else ("actor", "critic", "target_actor", "target_critic")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.manual_seed(int(z["hyper/init_seed"]))
        built = {}
        for net in order:
            built[net] = Network("deterministic_policy" if "actor" in net else "continuous_q_network", fx.S, fx.A, D_hidden=fx.H, head="mlp").state_dict()
    finally:
        torch.set_num_threads(threads)
    for net in fx.nets:
        src = built[net.replace("target_", "")]
        for k, v in src.items():
            assert np.array_equal(synth.thin(v.numpy()), z[f"init_thin/{net}/{k}"]), (net, k)
    # orthogonal_init's gains: pi "tanh" (5/3), q "linear" (1), every hidden layer "relu" (sqrt 2); biases zero
    w = built["actor"]["pi.weight"].double()
    assert torch.allclose(w @ w.t(), (5.0 / 3.0) ** 2 * torch.eye(fx.A, dtype=torch.float64), atol=1e-4)
    c = built[fx.critics()[0]]
    assert torch.allclose(c["q.weight"].double() @ c["q.weight"].double().t(), torch.ones(1, 1, dtype=torch.float64), atol=1e-4)
    w = c["l.weight"].double()
    assert torch.allclose(w @ w.t(), 2.0 * torch.eye(fx.H, dtype=torch.float64), atol=1e-3) and not c["l.bias"].any() and not c["e.bias"].any()


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_reproduces_the_reference_fixture(name):
    """Float64 against the reference's float32 run: values within 1e-5 of the tensor's largest entry (a handful of layers of at most
    1024-term float32 sums), scalars rtol 1e-5, gradients within 1e-5 of the tensor's largest entry -- the tolerances of test_iqn_cpu."""
    z = load(name)
    fx = D.Fixture(z)
    gamma = float(z["hyper/gamma"])
    std, clip = fx.noise_args()
    assert fx.records == (["r0", "r1", "r2"] if fx.kind == "td3" else ["r0"])
    for r in fx.records:
        b = fx.batch(r)
        assert b["state"].shape == (fx.B, fx.S) and b["action"].shape == (fx.B, fx.A)
        t = D.critic_update(fx.sd0["target_actor"], [fx.sd0[n] for n in fx.critics()], [fx.sd0[n] for n in fx.critics(True)], b["state"], b["action"], b["reward"],
                            b["next_state"], b["done"], fx.eps(r), gamma, std, clip)

        def close(ours, ref, what):
            ref = np.asarray(ref, dtype=np.float64)
            err = float(np.abs(np.asarray(ours, dtype=np.float64).reshape(ref.shape) - ref).max())
            assert err <= 1e-5 * max(float(np.abs(ref).max()), 1e-30), (r, what, err)

        close(t["next_action"], z[f"{r}/learn/next_action"], "next_action")
        close(t["y"], z[f"{r}/learn/target_q"], "y")
        close(t["q"][0], z[f"{r}/learn/q1"], "q1")
        np.testing.assert_allclose(float(t["max_Q"]), float(z[f"{r}/result/max_Q"]), rtol=1e-5)
        if fx.kind == "td3":
            close(t["q"][1], z[f"{r}/learn/q2"], "q2")
            np.testing.assert_allclose(float(t["loss"][0]), float(z[f"{r}/result/critic_loss1"]), rtol=1e-5)
            np.testing.assert_allclose(float(t["loss"][1]), float(z[f"{r}/result/critic_loss2"]), rtol=1e-5)
        else:
            np.testing.assert_allclose(float(t["loss"][0]), float(z[f"{r}/result/critic_loss"]), rtol=1e-5)
        for net, g in zip(fx.critics(), t["grads"]):
            for k, v in g.items():
                err = float(np.abs(fx.thin(v.numpy()) - z[f"{r}/grad/{net}/{k}"]).max())
                assert err <= 1e-5 * float(z[f"{r}/grad_absmax/{net}/{k}"]), (r, net, k, err)
        if not fx.has_actor_step(r):
            assert fx.kind == "td3" and int(z[f"{r}/num_learn"]) == 1 and float(z[f"{r}/result/actor_loss"]) == 0.0
            assert fx.unchanged(r, "actor") and all(fx.unchanged(r, n) for n in fx.nets if n.startswith("target_"))
            continue
        # the actor step uses critic 1 AFTER its step.  Every record starts from a fresh optimizer, so the truth takes that first Adam step
        # itself, in float64, from the gradients it has just computed -- in every fixture, thinned or not.
        c1 = fx.critics()[0]
        lr = float(z["hyper/critic_lr"])
        sd_c1 = D.adam_first_step(fx.sd0[c1], t["grads"][0], lr)
        # ... and lands on the reference's stepped critic within the caps of the agent tests: a first Adam step is lr * g / (|g| + eps), so a
        # float32 gradient next to zero may move a weight by up to 2 lr differently; at most 0.5 % of the weights further than 2e-5
        diff = np.concatenate([np.abs(fx.thin(v.numpy()).astype(np.float64) - z[f"{r}/sd1/{c1}/{k}"]).reshape(-1) for k, v in sd_c1.items()])
        assert diff.max() <= 2.1 * lr and (diff > 2e-5).mean() <= 0.005, (r, c1, diff.max(), (diff > 2e-5).mean())
        a = D.actor_update(fx.sd0["actor"], sd_c1, b["state"])
        close(a["action_pred"], z[f"{r}/learn/action_pred"], "action_pred")
        np.testing.assert_allclose(float(a["actor_loss"]), float(z[f"{r}/learn/actor_loss"]), rtol=1e-5)
        np.testing.assert_allclose(float(a["actor_loss"]), float(z[f"{r}/result/actor_loss"]), rtol=1e-5)
        for k, v in a["grads"].items():
            err = float(np.abs(fx.thin(v.numpy()) - z[f"{r}/grad/actor/{k}"]).max())
            assert err <= 1e-5 * float(z[f"{r}/grad_absmax/actor/{k}"]), (r, k, err)
        soft = fx.kind == "td3" and int(z[f"{r}/num_learn"]) > 0
        assert all(fx.unchanged(r, n) != soft for n in fx.nets if n.startswith("target_")), r
        if soft:
            # the soft update in the reference's own arithmetic, bit for bit, on every stored element (thinning picks the same elements of
            # the online net, of the target before and of the target after).  It is also what jh_td3_polyak implements: torch rounds the
            # Python scalars tau and (1 - tau) -- the latter formed in double -- to float32 and takes two float32 products and one sum.
            tau = float(z["hyper/tau"])
            for net in ("actor", "critic1", "critic2"):
                for k in fx.sd0[net]:
                    p, t0 = z[f"{r}/sd1/{net}/{k}"], fx.thin(fx.sd0["target_" + net][k])
                    want = D.polyak(torch.from_numpy(p), torch.from_numpy(np.ascontiguousarray(t0)), tau).numpy()
                    assert np.array_equal(want, z[f"{r}/sd1/target_{net}/{k}"]), (net, k)
                    mine = np.float32(tau) * p + np.float32(1.0 - tau) * t0
                    assert mine.dtype == np.float32 and np.array_equal(want.view(np.uint32), mine.view(np.uint32)), (net, k)
                    assert np.array_equal(D.polyak(torch.from_numpy(p), torch.from_numpy(np.ascontiguousarray(t0)), 1.0).numpy(), p)


def test_sweep_generators_keep_both_clamps_active_on_both_sides():
    assert D.NEXT_ACTION_SHAPES == ((1, 1), (7, 3), (128, 6), (1025, 17))
    for B, A in D.NEXT_ACTION_SHAPES:
        cases = D.next_action_cases(B, A)
        counts = np.asarray([D.clamps_active(z, eps) for z, eps in cases])
        if B * A >= 2:  # every case on its own
            assert (counts > 0).all(), (B, A, counts)
        else:           # one element sits on one side: the shape's two cases together
            assert len(cases) == 2 and (counts.sum(0) > 0).all(), (B, A, counts)
        for z, eps in cases:
            assert z.shape == (B, A) and z.dtype == np.float32 and eps.dtype == np.float32
            t64, t32 = D.next_action(z, eps, D.STD, D.CLIP), D.next_action(z, eps, D.STD, D.CLIP, torch.float32)
            assert float((t64 - t32.double()).abs().max()) <= 2e-7 and float(t64.abs().max()) <= 1.0
    for B in D.CRITIC_LOSS_B:
        for n in (1, 2):
            for variant in D.CRITIC_LOSS_VARIANTS:
                q, qn, r, d = D.critic_loss_case(B, n, variant)
                assert q.shape == (n, B) and qn.shape == (n, B)
                if variant == "all_done":
                    assert d.all()
                    np.testing.assert_array_equal(D.critic_loss(q, qn, r, d, 0.99)["y"].numpy(), r.astype(np.float64))
                if variant == "equal_targets" and n == 2:
                    assert np.array_equal(qn[0], qn[1])


def test_curve_fixture_was_made_with_the_config_the_gpu_test_runs():
    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_td3.json")) as f:
        fx = json.load(f)
    assert fx["config"] == CURVE_CONFIG and fx["seeds"] == [1, 2, 3]
    for kind in ("td3", "ddpg"):
        ref = fx[kind]["reference"]
        assert len(ref) == 3 and all(len(r) == CURVE_CONFIG["steps"] // CURVE_CONFIG["chunk"] for r in ref)
        start, end = np.mean([x[0] for x in ref]), np.mean([np.mean(x[-3:]) for x in ref])
        assert end > start + 0.3, (kind, start, end)  # the GPU test's assertion holds for the reference's own three seeds


UNSUPPORTED = [
    dict(head="cnn", state_size=(4, 84, 84)),
    dict(head="cnn"),
    dict(state_size=(4,)),
    dict(hidden_size=30),
    dict(actor="discrete_policy"),
    dict(critic="discrete_q_network"),
    dict(optim_config={"actor": "rmsprop", "critic": "adam", "actor_lr": 1e-3, "critic_lr": 1e-3}),
    dict(optim_config={"actor": "adam", "critic": "sgd", "actor_lr": 1e-3, "critic_lr": 1e-3}),
    dict(optim_config={"actor": "adam", "critic": "adam", "actor_lr": 1e-3, "critic_lr": 1e-3, "weight_decay": 0.1}),
]


@pytest.mark.parametrize("agent", ["td3", "ddpg"])
def test_configuration_errors_raise_before_any_gpu_use(agent):
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.ddpg import DDPG_ELIGIBLE
    from jorldy_amd.core.agent.td3 import TD3_ELIGIBLE

    for over in UNSUPPORTED:
        kw = dict(state_size=4, action_size=2)
        kw.update(over)
        with pytest.raises(ValueError, match="libjorldy_hip") as e:
            Agent(agent, **kw)
        assert (TD3_ELIGIBLE if agent == "td3" else DDPG_ELIGIBLE) in str(e.value)
