"""M-IQN on the GPU: jh_miqn_loss against the float64 truth of tests/miqn_truth.py (pinned to the reference's own learn() by
tests/test_miqn_cpu.py) and against the fixtures of tools/gen_golden_miqn.py; the forward arrangement jh_iqnnet_learn_forward_m with
IQN's backward and Adam against the float64 mirror network; then the whole agent: one learn() per fixture with the fixture's draws
injected in the native slot order, hipGraph replay against eager, fresh draws under replay, the configs' shapes, checkpoints."""
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import miqn_truth as M
from oracle import synth
from tests.util import f32, load, npy

pytestmark = pytest.mark.gpu

FIXTURES = ["miqn", "miqn_odd", "miqn_cartpole"]
NATIVE_SLOTS = [0, 3, 2]  # the reference's four draws -> online(state) for the loss, online(state) for the policy, target(next_state)
KEYS5 = ("loss", "epsilon", "max_Q", "max_logit", "min_logit")
TOL = 1e-5


# ----------------------------------------------------------------------------------------------- the loss kernel
def _fixture_inputs(z):
    d = {k: z[f"learn/{s}"] for k, s in (("logit", "logit"), ("logit_again", "logit_again"), ("target", "logit_target"))}
    d.update({k: z[f"learn/{k}"].reshape(-1) for k in ("action", "reward", "done")})
    d["tau"] = z["learn/tau"][0]
    return d, dict(gamma=float(z["hyper/gamma"]), alpha=float(z["hyper/alpha"]), tau_e=float(z["hyper/m_tau"]), l_0=float(z["hyper/l_0"]))


def _run_kernel(d, hy, stats=None):
    from jorldy_amd import ops

    g, st = ops.miqn_loss(f32(d["logit"]), f32(d["logit_again"]), f32(d["target"]), f32(d["action"]), f32(d["reward"]), f32(d["done"]), f32(d["tau"]), hy["gamma"],
                          hy["alpha"], hy["tau_e"], hy["l_0"], stats=stats)
    torch.cuda.synchronize()
    return npy(g), npy(st)


@pytest.mark.parametrize("name", FIXTURES)
def test_miqn_loss_matches_the_reference_fixture(name):
    from test_iqn_gpu import _check_stats, _others_are_zero

    z = load(name)
    d, hy = _fixture_inputs(z)
    grad, st = _run_kernel(d, hy, stats=torch.full((8,), -1.0, device="cuda"))
    _check_stats(st, {k: float(z[f"result/{k}"]) for k in ("loss", "max_Q", "max_logit", "min_logit")}, name)
    t = M.miqn_loss(**d, **hy)
    e = T.grad_vs_exact(grad, t["grad"], z["learn/d_logit"], TOL, f"{name} d(loss)/d(logit)")
    print(f"{name}: gradient |ours - fp64| / max = {e[0]:.3e} (reference fp32: {e[1]:.3e})")
    _others_are_zero(grad, d["action"])


@pytest.mark.parametrize("B,A,N,variant", M.SWEEP, ids=[f"B{c[0]}-A{c[1]}-N{c[2]}-{c[3]}" for c in M.SWEEP])
def test_miqn_loss_matches_float64_truth_over_a_sweep(B, A, N, variant):
    """`wide` and `tau1` are where 1 / tau_e amplifies the rounding of the quantile means: the float32 comparator carries the same
    amplification, the constant stays 1e-5."""
    from test_iqn_gpu import _check_stats, _others_are_zero

    d, hy = M.sweep_case(B, A, N, variant)
    grad, st = _run_kernel(d, hy, stats=torch.full((8,), -1.0, device="cuda"))
    t, t32 = M.miqn_loss(**d, **hy), M.miqn_loss(dtype=torch.float32, **d, **hy)
    _check_stats(st, t, f"B{B} A{A} N{N} {variant}")
    e = T.grad_vs_exact(grad, t["grad"], t32["grad"], TOL, "d(loss)/d(logit)")
    print(f"gradient |ours - fp64| / max = {e[0]:.3e} (torch-cpu-fp32: {e[1]:.3e})")
    _others_are_zero(grad, d["action"])


def test_miqn_loss_is_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B, A, N in ((32, 2, 64), (255, 6, 51), (7, 5, 33)):
        d, hy = M.sweep_case(B, A, N, "plain", seed=1)
        args = [f32(d[k]) for k in ("logit", "logit_again", "target", "action", "reward", "done", "tau")] + [hy[k] for k in ("gamma", "alpha", "tau_e", "l_0")]
        g1, s1 = ops.miqn_loss(*args)
        g2, s2 = ops.miqn_loss(*args)
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(s1, s2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            g3, s3 = ops.miqn_loss(*args)
        g3.fill_(7.0)
        s3.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, g3) and torch.equal(s1, s3)


def test_miqn_loss_clamps_out_of_range_actions():
    d, hy = M.sweep_case(7, 5, 33, "plain")
    wild = d["action"].copy()
    wild[0], wild[1] = -3.0, 11.0
    clamped = np.clip(wild, 0, 4)
    g_w, s_w = _run_kernel(dict(d, action=wild), hy)
    g_c, s_c = _run_kernel(dict(d, action=clamped), hy)
    assert np.array_equal(g_w, g_c) and np.array_equal(s_w, s_c)
    assert g_w[0, :, 0].any() and g_w[1, :, 4].any()


@pytest.mark.parametrize("bad", [dict(N=0), dict(N=257), dict(tau_e=0.0), dict(tau_e=-0.03), dict(l_0=0.5)], ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_miqn_loss_rejects_bad_arguments(bad):
    from jorldy_amd import _lib, ops

    N = bad.get("N", 4)
    hy = dict(M.HYPER, **{k: v for k, v in bad.items() if k != "N"})
    z = torch.zeros(2, N, 2, device="cuda")
    v = torch.zeros(2, device="cuda")
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.miqn_loss(z, z, z, v, v, v, torch.zeros(2, N, device="cuda"), hy["gamma"], hy["alpha"], hy["tau_e"], hy["l_0"])


# ----------------------------------------------------------------------------------------------- the forward arrangement
@pytest.mark.parametrize("S,A,H,E,N,B", M.NET_SHAPES)
def test_learn_forward_m_backward_and_adam_match_float64(S, A, H, E, N, B):
    """test_iqnnet_three_forwards_backward_and_adam_match_float64 with M-IQN's arrangement: slot 0 online(state) draw 0 (differentiated),
    slot 1 online(state) draw 1, slot 2 target(next_state) draw 2."""
    from jorldy_amd import _lib, ops
    from test_iqn_gpu import _fwd, _mirror64
    from test_rbnet_gpu import _force, _grads_vs_exact, _native_state

    ref64, ref32 = _mirror64(S, A, E, N, H, 0)
    tgt64, tgt32 = _mirror64(S, A, E, N, H, 100)
    nat = ops.IQNNet(S, A, E, N, H, B, "cuda:0")
    nat.import_state(ref32.state_dict(), nat.params)
    nat.import_state(tgt32.state_dict(), nat.target)
    lr = 1e-3
    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    g = torch.Generator().manual_seed(1)
    for it in range(2):
        _force(nat, truth, lambda step: nat.set_hyper(lr, 0.9, 0.999, 1e-8, step), it)
        x = torch.randn(2 * B, S, generator=g)
        tau = torch.rand(3, B, N, generator=g)
        x_dev, tau_dev = x.cuda(), tau.cuda()
        out = torch.empty(3, B, N, A, device="cuda")
        nat.learn_forward_m(x_dev, B, tau_dev, out)
        tn = tau.numpy()
        q0, q0_32 = _fwd(ref64, x[:B], tn[0]), _fwd(ref32, x[:B], tn[0])
        with torch.no_grad():
            q1, q1_32, q2, q2_32 = _fwd(ref64, x[:B], tn[1]), _fwd(ref32, x[:B], tn[1]), _fwd(tgt64, x[B:], tn[2]), _fwd(tgt32, x[B:], tn[2])
        T.vs_exact(out[0], q0, q0_32, TOL, f"step {it} online(state), draw 0")
        T.vs_exact(out[1], q1, q1_32, TOL, f"step {it} online(state), draw 1")
        T.vs_exact(out[2], q2, q2_32, TOL, f"step {it} target(next_state)")
        if it == 0:
            first = out.clone()
            single = nat.forward(x_dev[:B].contiguous(), 0, tau_dev[1].contiguous())
            assert torch.equal(single, first[1]), "slot 1 is a plain forward(state, online, draw 1)"
            iqn = torch.empty(3, B, N, A, device="cuda")
            nat.learn_forward(x_dev, B, tau_dev, iqn)  # IQN's arrangement: its slot 1 is online(next_state) under the same draw
            assert torch.equal(iqn[0], first[0]) and torch.equal(iqn[2], first[2]) and not torch.equal(iqn[1], first[1])
            nat.learn_forward_m(x_dev, B, tau_dev, out)  # the activations backward reads are back in place
            assert torch.equal(out, first)
        gl = torch.randn(B, N, A, generator=g) / (B * N)
        truth.opt64.zero_grad()
        truth.opt32.zero_grad()
        q0.backward(gl.double())
        q0_32.backward(gl)
        nat.backward(gl.cuda().contiguous())
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"step {it} ")
        nat.optim_step("adam", None)
        truth.step(None, raw, *_native_state(nat), tag=f"adam step {it}")
    nat.forward(x_dev[:B].contiguous(), 0, tau_dev[0].contiguous())  # a plain forward takes the activations away
    with pytest.raises(_lib.JhError, match="without a preceding"):
        nat.backward(gl.cuda().contiguous())


# ----------------------------------------------------------------------------------------------- the agent
def _agent_for(z, use_graph=True, lr=None, **over):
    from jorldy_amd.core.agent import Agent
    from test_agents_gpu import _h

    oc = {"name": "adam", "lr": _h(z, "lr") if lr is None else lr}
    if "hyper/optim_eps" in z.files and lr is None:
        oc["eps"] = _h(z, "optim_eps")
    kw = dict(state_size=int(_h(z, "S")), action_size=int(_h(z, "A")), num_sample=int(_h(z, "N")), embedding_dim=int(_h(z, "E")), optim_config=oc,
              alpha=_h(z, "alpha"), tau=_h(z, "m_tau"), l_0=_h(z, "l_0"), gamma=_h(z, "gamma"), buffer_size=256, batch_size=int(_h(z, "B")), start_train_step=0,
              target_update_period=10000, run_step=100000, device="cuda", use_graph=use_graph)
    kw.update(over)
    return Agent("m_iqn", **kw)


def _loaded_agent(z, **kw):
    from test_agents_gpu import _fill_from_fixture
    from test_iqn_gpu import _initial_weights

    agent = _agent_for(z, **kw)
    w0, wt = _initial_weights(z, agent)
    agent.network.load_state_dict(w0)
    agent.target_network.load_state_dict(wt)
    _fill_from_fixture(agent, z, False)
    return agent, w0, wt


@pytest.mark.parametrize("name", FIXTURES)
def test_miqn_agent_learn_matches_reference(name):
    """The assertions and caps of test_iqn_agent_learn_matches_reference, with the fixture's draws 0, 3 and 2 injected."""
    from jorldy_amd.core.agent.miqn import MIQN
    from test_agents_gpu import _h
    from test_iqn_gpu import _thin_cmp

    z = load(name)
    agent, w0, wt = _loaded_agent(z)
    assert type(agent) is MIQN and agent.backend == "native" and agent._net.H == 512 and agent._net.kind == "iqn"
    assert (agent.alpha, agent.tau, agent.l_0) == (0.9, 0.03, -1.0)
    agent._tau_inject = z["learn/tau"][NATIVE_SLOTS]
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    assert set(result) == set(KEYS5)
    for k in KEYS5:
        print(f"{name} result {k}: ours {result[k]!r} reference {float(z[f'result/{k}'])!r}")
        np.testing.assert_allclose(result[k], z[f"result/{k}"], rtol=1e-5, err_msg=k)
    lg = npy(agent._static["logits"])
    for i, k in enumerate(("logit", "logit_again", "logit_target")):  # same sampled rows, same draws, same forwards
        np.testing.assert_allclose(lg[i], z[f"learn/{k}"], rtol=1e-5, atol=1e-5, err_msg=k)
    lr = _h(z, "lr")
    _thin_cmp({k: npy(v) for k, v in w0.items()}, z, "sd0_thin/", tol=0.0, what="initial weights", only_stored=True)
    _thin_cmp({k: npy(v) for k, v in wt.items()}, z, "sdt_thin/", tol=0.0, what="target weights", only_stored=True)
    grads = {k: npy(v) for k, v in agent._net.export_state(agent._net.grads).items()}
    _thin_cmp(grads, z, "grad_thin/", scale_of=lambda k: z[f"grad_absmax/{k}"], tol=1e-5, what="d(loss)/d")
    for bucket, nm in ((agent._net.m, "exp_avg"), (agent._net.v, "exp_avg_sq")):
        _thin_cmp({k: npy(v) for k, v in agent._net.export_state(bucket).items()}, z, f"opt1_thin/{nm}/", tol=2e-5, what=nm)
    tot = bad = 0
    worst = 0.0
    stride = int(z["thin_stride"])
    for k, v in agent.network.state_dict().items():
        dd = np.abs(synth.thin(npy(v), stride=stride) - z[f"sd1_thin/{k}"])
        tot += dd.size
        bad += int((dd > 2e-5).sum())
        worst = max(worst, float(dd.max()))
    margins.leq(bad / tot, 0.005, "fraction of weights further than 2e-5 from the reference's")
    margins.leq(worst, 2.1 * lr, "worst weight difference vs the possible travel")


def test_miqn_graph_replay_equals_eager():
    """The assertions of test_iqn_graph_replay_equals_eager: 5 learn() calls with lr decay, captured against eager."""
    z = load("miqn")
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent, _, _ = _loaded_agent(z, use_graph=use_graph, lr=1e-3, run_step=1000)
        np.random.seed(7)
        out = []
        for it in range(5):
            r = agent.learn()
            agent.learning_rate_decay(10 * (it + 1))
            out.append(r["loss"])
        if use_graph:
            assert agent._graph is not None, "learn() was not captured"
        res.append((out, torch.cat([p.detach().reshape(-1) for p in agent.network.parameters()]).clone()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)


def test_replayed_learns_see_fresh_tau_draws():
    """Learning rate 0 and the same sampled rows: two consecutive replays differ only in their three tau draws -- and so does the loss;
    with the draws injected they give the same bits."""
    z = load("miqn")
    torch.manual_seed(0)
    agent, _, _ = _loaded_agent(z, lr=0.0, lr_decay=False)
    losses = []
    for it in range(4):
        np.random.seed(7)
        losses.append(agent.learn()["loss"])
    assert agent._graph is not None
    assert tuple(agent._static["tau"].shape) == (3, int(z["hyper/B"]), int(z["hyper/N"]))
    assert losses[2] != losses[3] and len(set(losses)) == 4
    agent._tau_inject = z["learn/tau"][NATIVE_SLOTS]
    fixed = []
    for it in range(2):
        np.random.seed(7)
        fixed.append(agent.learn()["loss"])
    assert fixed[0] == fixed[1] and fixed[0] not in losses


MIQN_SUPPORTED = [
    ("config.m_iqn.cartpole", dict(state_size=4, action_size=2)),
    ("config.m_iqn.mountaincar", dict(state_size=2, action_size=3)),
    ("config.m_iqn.pong_mlagent", dict(state_size=8, action_size=3)),
]


@pytest.mark.parametrize("label,kw", MIQN_SUPPORTED, ids=[c[0] for c in MIQN_SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(dict(network="iqn", optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}, buffer_size=64, batch_size=32, num_sample=64, embedding_dim=64,
                   sample_min=0.0, sample_max=1.0, alpha=0.9, tau=0.03, l_0=-1, device="cuda"), **kw)
    agent = Agent("m_iqn", **kw)
    assert agent.backend == "native" and agent.num_support == 64 and agent._net.H == 512
    state = np.random.randn(2, kw["state_size"]).astype(np.float32)
    for training in (True, False):  # epsilon 1: random; epsilon_eval 0: the network + jh_iqn_act
        a = agent.act(state, training)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))


def test_the_cnn_head_raises_at_construction():
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.iqn import IQN_ELIGIBLE

    with pytest.raises(ValueError) as e:
        Agent("m_iqn", state_size=(4, 84, 84), action_size=6, head="cnn", optim_config={"name": "adam", "lr": 1e-4}, device="cuda")
    assert IQN_ELIGIBLE in str(e.value) and "not on the native engine yet" in str(e.value)


def test_checkpoint_and_load_full_roundtrip(tmp_path):
    from test_agents_gpu import _fill_from_fixture

    z = load("miqn")
    a, _, _ = _loaded_agent(z)
    np.random.seed(3)
    a.learn()  # the checkpoint carries Adam moments and a step count
    a.update_target()  # load() gives both networks the checkpoint's weights
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert list(ckpt["network"].keys()) == list(M.KEYS)
    b = _agent_for(z)
    b.load(str(tmp_path))
    _fill_from_fixture(b, z, False)
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, b.network.state_dict()[k]) and torch.equal(v, b.target_network.state_dict()[k]), k
    res = []
    for ag in (a, b):
        np.random.seed(11)
        ag._tau_inject = z["learn/tau"][NATIVE_SLOTS]
        res.append(ag.learn())
        ag._tau_inject = None
    for k in KEYS5:
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=1e-6, err_msg=k)
    flat = lambda ag: torch.cat([p.detach().reshape(-1) for p in ag.network.parameters()])
    torch.testing.assert_close(flat(b), flat(a), rtol=1e-5, atol=1e-6)
    c = _agent_for(z)
    c.sync_in(a.sync_out()["weights"])
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, c.network.state_dict()[k]), k
    # save_full / load_full: buffer, counters and the RNG states (numpy: the sampled rows; torch's on the device: the tau draws) survive
    (tmp_path / "full").mkdir()
    a.save_full(str(tmp_path / "full"))
    want = a.learn()
    d = _agent_for(z)
    d.load_full(str(tmp_path / "full"))
    got = d.learn()
    for k in ("loss", "max_Q", "max_logit", "min_logit"):
        np.testing.assert_allclose(got[k], want[k], rtol=1e-6, err_msg=f"load_full {k}")
