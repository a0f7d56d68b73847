"""Munchausen DQN on the GPU: the loss kernel (jh_mdqn_loss) against the reference's own learn() (fixtures of tools/gen_golden_mdqn.py)
and against the float64 truth of tests/mdqn_truth.py (pinned to those fixtures by tests/test_mdqn_cpu.py); the forward that runs the
target network on both halves of the batch (jh_rbnet_learn_forward_m) against float64 mirrors; then the whole agent: one learn()
against the reference, hipGraph replay against eager, the configs' shapes, checkpoints, and the learning curve of config.m_dqn.cartpole
next to the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import mdqn_truth as M
from tests.util import f32, load, npy

pytestmark = pytest.mark.gpu

FIXTURES = ["mdqn", "mdqn_odd", "mdqn_cartpole"]
TOL = 1e-5
ARGS = ("q", "q_target", "q_next_target", "action", "reward", "done")


def _fixture_inputs(z):
    d = dict(q=z["learn/q_all"], q_target=z["learn/target_q_state"], q_next_target=z["learn/next_target_q"])
    d.update({k: z[f"learn/{k}"].reshape(-1) for k in ("action", "reward", "done")})
    h = dict(gamma=float(z["hyper/gamma"]), alpha=float(z["hyper/alpha"]), tau=float(z["hyper/m_tau"]), l_0=float(z["hyper/l_0"]))
    return d, h


def _run_kernel(d, h):
    from jorldy_amd import ops

    g, st = ops.mdqn_loss(*[f32(d[k]) for k in ARGS], h["gamma"], h["alpha"], h["tau"], h["l_0"], stats=torch.full((4,), -1.0, device="cuda"))
    torch.cuda.synchronize()
    return npy(g), npy(st)


def _check_stats(st, want, what):
    for i, k in enumerate(("loss", "max_Q", "mun_mean")):
        print(f"{what} {k}: ours {st[i]!r} want {want[k]!r}")
        np.testing.assert_allclose(st[i], want[k], rtol=1e-5, err_msg=f"{what} {k}")
    assert st[3] == 0.0, "arrival mark"


def _off_action_entries_are_zero(grad, action):
    B, A = grad.shape
    other = np.ones((B, A), bool)
    other[np.arange(B), np.clip(np.asarray(action).astype(np.int64), 0, A - 1)] = False
    assert not grad[other].any(), "entries of the actions not taken must be written as zeros"


# ----------------------------------------------------------------------------------------------- the loss kernel
@pytest.mark.parametrize("name", FIXTURES)
def test_mdqn_loss_matches_the_reference_fixture(name):
    z = load(name)
    d, h = _fixture_inputs(z)
    grad, st = _run_kernel(d, h)
    _check_stats(st, dict(loss=float(z["result/loss"]), max_Q=float(z["result/max_Q"]), mun_mean=float(z["learn/munchausen_term"].mean(dtype=np.float64))), name)
    t = M.mdqn_truth(**d, **h)
    e = T.grad_vs_exact(grad, t["grad"], z["learn/d_q_all"], TOL, f"{name} d(loss)/d(q)")
    print(f"{name}: gradient |ours - fp64| / max = {e[0]:.3e} (reference fp32: {e[1]:.3e})")
    _off_action_entries_are_zero(grad, d["action"])


@pytest.mark.parametrize("B,A,variant", M.SWEEP, ids=[f"B{c[0]}-A{c[1]}-{c[2]}" for c in M.SWEEP])
def test_mdqn_loss_matches_float64_truth_over_a_sweep(B, A, variant):
    d, h = M.sweep_case(B, A, variant)
    grad, st = _run_kernel(d, h)
    t, t32 = M.mdqn_truth(**d, **h), M.mdqn_truth(dtype=torch.float32, **d, **h)
    _check_stats(st, t, f"B{B} A{A} {variant}")
    e = T.grad_vs_exact(grad, t["grad"], t32["grad"], TOL, "d(loss)/d(q)")
    print(f"gradient |ours - fp64| / max = {e[0]:.3e} (torch-cpu-fp32: {e[1]:.3e})")
    _off_action_entries_are_zero(grad, d["action"])
    if variant == "flat":
        assert not t["clipped"].any()
    if A == 1:
        assert not t["log_policy"].any() and st[2] == 0.0  # one action: the log-policy is exactly 0


@pytest.mark.parametrize("B,A", M.BOTH_SIDES)
def test_mdqn_loss_on_rows_on_both_sides_of_the_clip_and_of_the_huber_knee(B, A):
    d, h = M.sweep_case(B, A, "plain")
    t, t32 = M.mdqn_truth(**d, **h), M.mdqn_truth(dtype=torch.float32, **d, **h)
    assert t["clipped"].any() and not t["clipped"].all()
    assert t["linear"].any() and not t["linear"].all()
    grad, st = _run_kernel(d, h)
    _check_stats(st, t, f"B{B} A{A}")
    T.grad_vs_exact(grad, t["grad"], t32["grad"], TOL, "d(loss)/d(q)")
    _off_action_entries_are_zero(grad, d["action"])


def test_mdqn_loss_clamps_actions_into_range():
    d, h = M.sweep_case(32, 5, "plain")
    d["action"] = d["action"].copy()
    d["action"][0], d["action"][1] = -3.0, 9.0
    grad, st = _run_kernel(d, h)
    t = M.mdqn_truth(**d, **h)
    _check_stats(st, t, "clamped actions")
    T.grad_vs_exact(grad, t["grad"], None, TOL, "d(loss)/d(q)")
    assert grad[0, 0] != 0 and grad[1, 4] != 0


def test_mdqn_loss_is_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B, A in ((32, 2), (257, 6), (7, 5)):
        d, h = M.sweep_case(B, A, "plain", seed=1)
        args = [f32(d[k]) for k in ARGS] + [h["gamma"], h["alpha"], h["tau"], h["l_0"]]
        g1, s1 = ops.mdqn_loss(*args)
        g2, s2 = ops.mdqn_loss(*args)
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(s1, s2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            g3, s3 = ops.mdqn_loss(*args)
        g3.fill_(7.0)
        s3.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, g3) and torch.equal(s1, s3)


def test_mdqn_loss_rejects_bad_arguments():
    from jorldy_amd import _lib as L
    from jorldy_amd import ops

    q = torch.zeros(2, 3, device="cuda")
    v = torch.zeros(2, device="cuda")
    with pytest.raises(L.JhError):
        ops.mdqn_loss(q, q, q, v, v, v, 0.99, 0.9, 0.0, -1.0)  # tau = 0
    with pytest.raises(L.JhError):
        ops.mdqn_loss(q, q, q, v, v, v, 0.99, 0.9, 0.03, 0.5)  # l_0 > 0
    g, st = torch.empty_like(q), torch.empty(4, device="cuda")
    with pytest.raises(L.JhError):  # a null pointer
        L.check(L.load().jh_mdqn_loss(L.ctx(0), 2, 3, L.ptr(q), L.ptr(None), L.ptr(q), L.ptr(v), L.ptr(v), L.ptr(v), 0.99, 0.9, 0.03, -1.0, L.ptr(g), L.ptr(st),
                                      L.stream_ptr()))
    with pytest.raises(L.JhError):
        L.check(L.load().jh_mdqn_loss(L.ctx(0), 0, 3, L.ptr(q), L.ptr(q), L.ptr(q), L.ptr(v), L.ptr(v), L.ptr(v), 0.99, 0.9, 0.03, -1.0, L.ptr(g), L.ptr(st),
                                      L.stream_ptr()))


# ----------------------------------------------------------------------------------------------- online(s), target(s), target(s')
M_FORWARD_CASES = [("q", "mlp", 4, 3, 64), ("dueling", "mlp", 4, 3, 64), ("q", "cnn", (4, 44, 52), 6, 32), ("dueling", "cnn", (4, 44, 52), 6, 32)]


@pytest.mark.parametrize("kind,head,S,A,H", M_FORWARD_CASES)
def test_learn_forward_m_and_backward_match_float64(kind, head, S, A, H):
    from jorldy_amd import _lib as L
    from test_rbnet_gpu import _grads_vs_exact, _inputs, _mk_kind

    B = 8  # = max_batch: the target slot holds B rows until reserve_target_rows
    (ref64, ref32), (tgt64, tgt32), nat = _mk_kind(kind, head, S, A, H, B)
    g = torch.Generator().manual_seed(1)
    x_dev, x64 = _inputs(head, S, 2 * B, g)
    out = torch.full((3, B, A, 1), -7.0, device="cuda")
    with pytest.raises(L.JhError):  # no room for 2B target rows yet
        nat.learn_forward_m(x_dev, B, None, out)
    assert bool((out == -7.0).all())
    with pytest.raises(L.JhError):
        nat.reserve_target_rows(2 * B + 1)  # more than the im2col tables cover
    nat.reserve_target_rows(2 * B)
    nat.reserve_target_rows(B)  # never shrinks
    nat.learn_forward_m(x_dev, B, None, out)
    x32 = x64.float()
    q0, q0_32 = ref64(x64[:B]), ref32(x32[:B])
    with torch.no_grad():
        q1, q1_32, q2, q2_32 = tgt64(x64[:B]), tgt32(x32[:B]), tgt64(x64[B:]), tgt32(x32[B:])
    T.vs_exact(out[0, :, :, 0], q0, q0_32, TOL, "online(state)")
    T.vs_exact(out[1, :, :, 0], q1, q1_32, TOL, "target(state)")
    T.vs_exact(out[2, :, :, 0], q2, q2_32, TOL, "target(next_state)")
    gl = torch.randn(B, A, generator=g) / B
    q0.backward(gl.double())
    q0_32.backward(gl)
    nat.backward(gl.cuda().contiguous())
    _grads_vs_exact(nat, ref64, ref32)
    # learn_forward still computes what it did, on the grown slot
    out2 = torch.empty(3, B, A, 1, device="cuda")
    nat.learn_forward(x_dev, B, None, out2)
    T.vs_exact(out2[0, :, :, 0], q0, q0_32, TOL, "learn_forward online(state)")
    T.vs_exact(out2[2, :, :, 0], q2, q2_32, TOL, "learn_forward target(next_state)")


def test_learn_forward_m_refuses_a_noisy_network():
    from jorldy_amd import _lib as L
    from jorldy_amd import ops

    nat = ops.RainbowNet(4, 3, 11, 32, "mlp", 8, "cuda:0", kind="rainbow")
    nat.reserve_target_rows(16)
    x = torch.zeros(16, 4, device="cuda")
    noise = torch.zeros(3, nat.noise_len, device="cuda")
    with pytest.raises(L.JhError):
        nat.learn_forward_m(x, 8, noise, torch.empty(3, 8, 3, 11, device="cuda"))


# ----------------------------------------------------------------------------------------------- the agent
def _agent_for(z, use_graph=True, lr=None, **over):
    from jorldy_amd.core.agent import Agent
    from test_agents_gpu import _h

    kw = dict(state_size=int(_h(z, "S")), action_size=int(_h(z, "A")), hidden_size=int(_h(z, "H")), network=str(z["hyper/network"]),
              optim_config={"name": "adam", "lr": _h(z, "lr") if lr is None else lr}, alpha=_h(z, "alpha"), tau=_h(z, "m_tau"), l_0=_h(z, "l_0"),
              gamma=_h(z, "gamma"), buffer_size=256, batch_size=int(_h(z, "B")), start_train_step=0, target_update_period=10000, run_step=100000, device="cuda",
              use_graph=use_graph)
    kw.update(over)
    return Agent("m_dqn", **kw)


def _initial_weights(z, agent):
    """-> (online, target) state dicts: stored whole, or regenerated from the recipe seed (the wide fixture stores them thinned)."""
    from oracle import synth
    from test_agents_gpu import _sd

    if "recipe_seed" not in z.files:
        return _sd(z, "sd0/"), _sd(z, "sdt/")
    shapes = {k: v.shape for k, v in agent.network.state_dict().items()}
    seed = int(z["recipe_seed"])
    return ({k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed).items()},
            {k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed + 1).items()})


@pytest.mark.parametrize("name", FIXTURES)
def test_mdqn_agent_learn_matches_reference(name):
    from oracle import synth
    from test_agents_gpu import _cmp_sd, _fill_from_fixture, _h, _sd
    from test_baseline_width_gpu import _thin_cmp

    z = load(name)
    agent = _agent_for(z)
    assert agent.backend == "native" and (agent.alpha, agent.tau, agent.l_0) == (0.9, 0.03, -1)
    w0, wt = _initial_weights(z, agent)
    agent.network.load_state_dict(w0)
    agent.target_network.load_state_dict(wt)
    _fill_from_fixture(agent, z, False)
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    assert set(result) == {"loss", "epsilon", "max_Q"}
    for k in ("loss", "epsilon", "max_Q"):
        print(f"{name} result {k}: ours {result[k]!r} reference {float(z[f'result/{k}'])!r}")
        np.testing.assert_allclose(result[k], z[f"result/{k}"], rtol=1e-5, err_msg=k)
    B = int(_h(z, "B"))
    lg = npy(agent._static["logits"]).reshape(3, B, -1)
    for i, k in enumerate(("q_all", "target_q_state", "next_target_q")):  # same sampled rows, same forwards
        np.testing.assert_allclose(lg[i], z[f"learn/{k}"], rtol=1e-5, atol=1e-5, err_msg=k)
    lr = _h(z, "lr")
    if "recipe_seed" not in z.files:
        _cmp_sd(agent.network, _sd(z, "sd1/"), lr, 1)
        return
    _thin_cmp({k: npy(v) for k, v in w0.items()}, z, "sd0_thin/", tol=0.0, what="initial weights")
    _thin_cmp({k: npy(v) for k, v in wt.items()}, z, "sdt_thin/", tol=0.0, what="target weights")
    grads = {k: npy(v) for k, v in agent._net.export_state(agent._net.grads).items()}
    _thin_cmp(grads, z, "grad_thin/", scale_of=lambda k: z[f"grad_absmax/{k}"], tol=1e-5, what="d(loss)/d")
    for bucket, nm in ((agent._net.m, "exp_avg"), (agent._net.v, "exp_avg_sq")):
        _thin_cmp({k: npy(v) for k, v in agent._net.export_state(bucket).items()}, z, f"opt1_thin/{nm}/", tol=2e-5, what=nm)
    tot = bad = 0
    worst = 0.0
    for k, v in agent.network.state_dict().items():
        dd = np.abs(synth.thin(npy(v)) - z[f"sd1_thin/{k}"])
        tot += dd.size
        bad += int((dd > 2e-5).sum())
        worst = max(worst, float(dd.max()))
    margins.leq(bad / tot, 0.005, "fraction of weights further than 2e-5 from the reference's")
    margins.leq(worst, 2.1 * lr, "worst weight difference vs the possible travel")


def test_mdqn_graph_replay_equals_eager():
    """The assertions of test_td_agents_graph_replay_equals_eager, for MDQN."""
    from test_agents_gpu import _fill_from_fixture, _sd

    z = load("mdqn")
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent = _agent_for(z, use_graph=use_graph, lr=1e-3, run_step=1000)
        agent.network.load_state_dict(_sd(z, "sd0/"))
        agent.target_network.load_state_dict(_sd(z, "sdt/"))
        _fill_from_fixture(agent, z, False)
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


M_SUPPORTED = [
    ("config.m_dqn.cartpole", dict(state_size=4, action_size=2)),
    ("config.m_dqn.mountaincar", dict(state_size=2, action_size=3)),
    ("config.m_dqn.pong_mlagent", dict(state_size=8, action_size=3)),
    ("config.m_dqn.atari", dict(state_size=(4, 84, 84), action_size=6, head="cnn")),
    ("config.m_dqn.procgen", dict(state_size=(3, 64, 64), action_size=15, head="cnn")),
]


@pytest.mark.parametrize("label,kw", M_SUPPORTED, ids=[c[0] for c in M_SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(dict(hidden_size=64, optim_config={"name": "adam", "lr": 1e-4}, buffer_size=64, batch_size=8, device="cuda"), **kw)
    agent = Agent("m_dqn", **kw)
    assert agent.backend == "native" and (agent.alpha, agent.tau, agent.l_0) == (0.9, 0.03, -1)
    S = kw["state_size"]
    state = np.random.randint(0, 256, size=(2,) + tuple(S), dtype=np.uint8) if isinstance(S, tuple) else np.random.randn(2, S).astype(np.float32)
    for training in (True, False):  # epsilon 1: random; epsilon_eval 0: the network
        a = agent.act(state, training)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))


def test_unsupported_configurations_raise_at_construction():
    from jorldy_amd.core.agent import Agent

    base = dict(state_size=4, action_size=2, hidden_size=64, optim_config={"name": "adam", "lr": 1e-4}, device="cuda")
    with pytest.raises(ValueError) as e:
        Agent("m_dqn", network="rainbow", **base)
    assert "libjorldy_hip" in str(e.value) and "discrete_q_network" in str(e.value)
    with pytest.raises(ValueError) as e:
        Agent("m_dqn", tau=0.0, **base)
    assert "tau=0.0" in str(e.value)
    with pytest.raises(ValueError) as e:
        Agent("m_dqn", l_0=1, **base)
    assert "l_0=1" in str(e.value)
    with pytest.raises(ValueError) as e:
        Agent("m_dqn", hidden_size=30, **{k: v for k, v in base.items() if k != "hidden_size"})
    assert "libjorldy_hip" in str(e.value)
    with pytest.raises(ValueError):
        Agent("m_dqn", **dict(base, optim_config={"name": "sgd", "lr": 1e-4}))


def test_checkpoint_and_weight_sync_roundtrip(tmp_path):
    from test_agents_gpu import _fill_from_fixture, _sd

    z = load("mdqn")
    a = _agent_for(z)
    a.network.load_state_dict(_sd(z, "sd0/"))
    a.target_network.load_state_dict(_sd(z, "sdt/"))
    _fill_from_fixture(a, z, False)
    np.random.seed(3)
    a.learn()  # the checkpoint carries Adam moments and a step count
    a.update_target()  # load() gives both networks the checkpoint's weights (dqn.py:190-199)
    a.save(str(tmp_path))
    b = _agent_for(z)
    b.load(str(tmp_path))
    _fill_from_fixture(b, z, False)
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, b.network.state_dict()[k]) and torch.equal(v, b.target_network.state_dict()[k]), k
    res = []
    for ag in (a, b):
        np.random.seed(11)
        res.append(ag.learn())
    for k in ("loss", "epsilon", "max_Q"):
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=1e-6, err_msg=k)
    flat = lambda ag: torch.cat([p.detach().reshape(-1) for p in ag.network.parameters()])
    torch.testing.assert_close(flat(b), flat(a), rtol=1e-5, atol=1e-6)
    c = _agent_for(z)
    c.sync_in(a.sync_out()["weights"])
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, c.network.state_dict()[k]), k


# ----------------------------------------------------------------------------------------------- learning curve
CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, hidden=512, batch=32, alpha=0.9, tau=0.03, l_0=-1, lr=1e-4, gamma=0.99,
                    epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


def test_mdqn_cartpole_learning_curve_tracks_the_reference():
    """config.m_dqn.cartpole in the single-mode loop of test_learning_curve_gpu._dqn_curve, three seeds, next to the curve of the REAL
    reference agent on the oracle's bit-identical CartPole (tests/golden/curves_reference_mdqn.json, tools/gen_golden_mdqn.py).  The
    reference's own three seeds go from 21.7 steps per episode (first two chunks) to 261 (last four): they satisfy all three of the DQN
    curve test's assertions, so all three are kept: both start near random play, both learn (end > 4 x start), and the ends lie
    within a factor 2 of each other."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from test_learning_curve_gpu import DQN_CHUNK, DQN_RUN_STEP, DQN_STEPS, _dqn_curve

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curves_reference_mdqn.json")) as f:
        fx = json.load(f)
    c = CURVE_CONFIG
    assert fx["mdqn_cartpole"]["config"] == c
    assert (c["steps"], c["run_step"], c["chunk"]) == (DQN_STEPS, DQN_RUN_STEP, DQN_CHUNK)
    ref = fx["mdqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == DQN_STEPS // DQN_CHUNK for r in ref)

    def gpu_env(seed):
        env = ops.CartPoleVec(1, seed=1000 + seed)
        return env, env.obs().copy()

    def gpu_step(env, action):
        nxt, rew, done = env.step(action)
        return nxt.copy(), rew.reshape(1, 1).astype(np.float64), done.reshape(1, 1).astype(bool), env.obs().copy()

    make = lambda: Agent("m_dqn", state_size=4, action_size=2, hidden_size=c["hidden"], network="discrete_q_network", alpha=c["alpha"], tau=c["tau"], l_0=c["l_0"],
                         optim_config={"name": "adam", "lr": c["lr"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"],
                         epsilon_min=c["epsilon_min"], explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"],
                         start_train_step=c["start"], target_update_period=c["target"], lr_decay=c["lr_decay"], run_step=c["run_step"], device="cuda")
    gpu = [_dqn_curve(make, gpu_env, gpu_step, s) for s in (1, 2, 3)]
    print(json.dumps({"steps": DQN_STEPS, "chunk": DQN_CHUNK, "metric": "mean episode length per 1000 env steps (max 500)", "hip": gpu, "reference": ref}))
    g_start, g_end = np.mean([np.mean(x[:2]) for x in gpu]), np.mean([np.mean(x[-4:]) for x in gpu])
    c_start, c_end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    print(f"M-DQN episode length: HIP {g_start:.1f} -> {g_end:.1f}, reference {c_start:.1f} -> {c_end:.1f}")
    assert g_start < 40 and c_start < 40  # random policy: ~22 steps
    assert g_end > 4 * g_start and c_end > 4 * c_start  # both learn
    assert 0.5 * c_end <= g_end <= 2.0 * c_end
