"""QR-DQN on the GPU: the quantile-Huber loss kernel (jh_qr_loss) and the acting kernel (jh_quantile_act) against the reference's own
learn() (fixtures of tools/gen_golden_qrdqn.py) and against the float64 truth of tests/qr_truth.py (pinned to those fixtures by
tests/test_qrdqn_cpu.py), then the whole agent: one learn() against the reference, hipGraph replay against eager, acting in the
reference's draw order, the configs' shapes, checkpoints, and the learning curve of config.qrdqn.cartpole next to the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import qr_truth as Q
from tests.util import cu, f32, load, npy

pytestmark = pytest.mark.gpu

FIXTURES = ["qrdqn", "qrdqn_odd", "qrdqn_cartpole"]
TOL = 1e-5


def _tau(N, device="cuda"):
    from jorldy_amd.core.agent.qrdqn import quantile_midpoints

    return quantile_midpoints(N).to(device)


def _fixture_inputs(z):
    N, B = int(z["tau"].size), int(z["learn/logit"].shape[0])
    d = {k: z[f"learn/{s}"].reshape(B, -1, N) for k, s in (("logit", "logit"), ("next_online", "logit_next"), ("target", "logit_target"))}
    d.update({k: z[f"learn/{k}"].reshape(-1) for k in ("action", "reward", "done")})
    return d


def _run_kernel(d, tau, gamma, stats=None):
    from jorldy_amd import ops

    g, st = ops.qr_loss(f32(d["logit"]), f32(d["next_online"]), f32(d["target"]), f32(d["action"]), f32(d["reward"]), f32(d["done"]), tau, gamma, stats=stats)
    torch.cuda.synchronize()
    return npy(g), npy(st)


def _truth_following_near_ties(d, tau, gamma, grad):
    """Float64 truth; on rows whose two best quantile means of online(s') are closer than two fp32 sums of N terms can be off by
    (Q.qr_truth: gap <= gap_bound) either of the two is a correct selection, and the truth takes the one the kernel's gradient row
    shows.  Everywhere else the selection is the float64 one, so a wrong a* shows up in the loss and the gradient.
    -> (truth, number of such rows)."""
    t = Q.qr_truth(tau=tau, gamma=gamma, **d)
    near = np.nonzero(t["gap"] <= t["gap_bound"])[0]
    if near.size == 0:
        return t, 0
    qn = np.asarray(d["next_online"], dtype=np.float64).mean(-1)
    alt = t["a_star"].copy()
    alt[near] = np.argsort(-qn[near], axis=-1, kind="stable")[:, 1]
    t_alt = Q.qr_truth(tau=tau, gamma=gamma, a_star=alt, **d)
    pick = t["a_star"].copy()
    for b in near:
        if np.abs(grad[b] - t_alt["grad"][b]).max() < np.abs(grad[b] - t["grad"][b]).max():
            pick[b] = alt[b]
    return Q.qr_truth(tau=tau, gamma=gamma, a_star=pick, **d), int(near.size)


def _check_stats(st, want, what):
    for i, k in enumerate(("loss", "max_Q", "max_logit", "min_logit")):
        print(f"{what} {k}: ours {st[i]!r} want {want[k]!r}")
        np.testing.assert_allclose(st[i], want[k], rtol=1e-5, err_msg=f"{what} {k}")
    assert st[4] == 0.0 and st[5] == 0.0 and st[6] == 0.0 and st[7] == 0.0


# ----------------------------------------------------------------------------------------------- the loss kernel
@pytest.mark.parametrize("name", FIXTURES)
def test_qr_loss_matches_the_reference_fixture(name):
    z = load(name)
    d = _fixture_inputs(z)
    gamma = float(z["hyper/gamma"])
    tau = _tau(int(z["tau"].size))
    assert np.array_equal(npy(tau), z["tau"])
    grad, st = _run_kernel(d, tau, gamma, stats=torch.full((8,), -1.0, device="cuda"))
    _check_stats(st, {k: float(z[f"result/{k}"]) for k in ("loss", "max_Q", "max_logit", "min_logit")}, name)
    t, near = _truth_following_near_ties(d, z["tau"], gamma, grad)
    assert near == 0
    assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(-1))
    e = T.grad_vs_exact(grad, t["grad"], z["learn/d_logit"].reshape(grad.shape), TOL, f"{name} d(loss)/d(logit)")
    print(f"{name}: gradient |ours - fp64| / max = {e[0]:.3e} (reference fp32: {e[1]:.3e})")
    act = d["action"].astype(np.int64)
    other = np.ones(grad.shape[:2], bool)
    other[np.arange(grad.shape[0]), act] = False
    assert not grad[other].any(), "rows of the actions not taken must be written as zeros"


@pytest.mark.parametrize("B,A,N,variant", Q.SWEEP, ids=[f"B{c[0]}-A{c[1]}-N{c[2]}-{c[3]}" for c in Q.SWEEP])
def test_qr_loss_matches_float64_truth_over_a_sweep(B, A, N, variant):
    d = Q.sweep_case(B, A, N, variant)
    tau = _tau(N)
    grad, st = _run_kernel(d, tau, 0.99, stats=torch.full((8,), -1.0, device="cuda"))
    t, near = _truth_following_near_ties(d, npy(tau), 0.99, grad)
    print(f"rows with a near-tie of the two best next actions: {near} of {B}")
    assert near <= 0.01 * B
    _check_stats(st, t, f"B{B} A{A} N{N} {variant}")
    e = T.grad_vs_exact(grad, t["grad"], None, TOL, "d(loss)/d(logit)")
    print(f"gradient |ours - fp64| / max = {e[0]:.3e}")
    act = np.clip(d["action"].astype(np.int64), 0, A - 1)
    other = np.ones((B, A), bool)
    other[np.arange(B), act] = False
    assert not grad[other].any()


def test_qr_loss_is_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B, A, N in ((32, 2, 200), (255, 6, 51), (7, 5, 33)):
        d = Q.sweep_case(B, A, N, "plain", seed=1)
        tau = _tau(N)
        args = [f32(d[k]) for k in ("logit", "next_online", "target", "action", "reward", "done")]
        g1, s1 = ops.qr_loss(*args, tau, 0.99)
        g2, s2 = ops.qr_loss(*args, tau, 0.99)
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(s1, s2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            g3, s3 = ops.qr_loss(*args, tau, 0.99)
        g3.fill_(7.0)
        s3.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, g3) and torch.equal(s1, s3)


def test_qr_loss_rejects_out_of_range_sizes():
    from jorldy_amd import _lib, ops

    z = torch.zeros(2, 2, 257, device="cuda")
    v = torch.zeros(2, device="cuda")
    with pytest.raises(_lib.JhError):
        ops.qr_loss(z, z, z, v, v, v, torch.zeros(257, device="cuda"), 0.99)


# ----------------------------------------------------------------------------------------------- the acting kernel
@pytest.mark.parametrize("R", [1, 5, 64])
@pytest.mark.parametrize("N", [1, 200])
def test_quantile_act_matches_numpy(R, N):
    from jorldy_amd import ops

    A = 4
    rs = np.random.RandomState(100 * R + N)
    lg = rs.randn(R, A, N).astype(np.float32)
    lg[0, 1] = lg[0, 3] = np.abs(lg[0]).max(0) + 1.0  # two identical rows that are the maximum: the first one wins
    if R > 2:
        lg[2, 0] = lg[2, 2] = np.abs(lg[2]).max(0) + 1.0
    q64 = lg.astype(np.float64).mean(-1)
    top = np.sort(q64, -1)
    clear = (top[:, -1] - top[:, -2]) > 2.0 * N * 2.0 ** -24 * np.abs(lg).reshape(R, -1).max(-1)
    clear[0] = True  # exact ties: identical rows give identical sums
    if R > 2:
        clear[2] = True
    assert clear.all()
    want = q64.argmax(-1)
    assert want[0] == 1 and (R <= 2 or want[2] == 0)
    act, q, q_all = ops.quantile_act(cu(lg), want_q_all=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(npy(q_all), q64, rtol=1e-5, atol=1e-6)
    assert np.array_equal(npy(act), want)
    assert np.array_equal(npy(q), npy(q_all)[np.arange(R), want])
    # epsilon path: the host's draws decide, q_taken follows the action taken
    eps = np.full(R, 0.5, np.float32)
    u = rs.rand(R)
    u[0] = 0.9  # at least one greedy row ...
    if R > 1:
        u[1] = 0.1  # ... and one random one
    ra = rs.randint(0, A, size=R).astype(np.int64)
    act2, q2, _ = ops.quantile_act(cu(lg), eps=eps, u=u, rand_action=ra)
    torch.cuda.synchronize()
    taken = np.where(u < eps, ra, want)
    assert np.array_equal(npy(act2), taken)
    assert np.array_equal(npy(q2), npy(q_all)[np.arange(R), taken])
    out = (torch.full((R,), -1, dtype=torch.int64, device="cuda"), torch.zeros(R, device="cuda"))
    ops.quantile_act(cu(lg), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(npy(out[0]), want)


# ----------------------------------------------------------------------------------------------- one algorithm, two layouts
# QR-DQN's entries read a row block as [A][N] with tau [N], IQN's as [N][A] with tau [B][N].  The same numbers through both give the
# same bits: sums, first maxima and the Bellman image do not depend on where an element lies in memory.
@pytest.mark.parametrize("B,A,N", [(1, 1, 1), (3, 2, 8), (32, 6, 65), (3, 18, 256), (255, 6, 51)])
def test_qr_loss_and_iqn_loss_are_one_algorithm(B, A, N):
    from jorldy_amd import ops

    assert (B, A, N, "plain") in Q.SWEEP
    d = Q.sweep_case(B, A, N, "plain")
    tau = _tau(N)
    am = [f32(d[k]) for k in ("logit", "next_online", "target")]
    sm = [x.transpose(1, 2).contiguous() for x in am]
    vec = [f32(d[k]) for k in ("action", "reward", "done")]
    g_qr, s_qr = ops.qr_loss(*am, *vec, tau, 0.99, stats=torch.full((8,), -1.0, device="cuda"))
    g_iqn, s_iqn = ops.iqn_loss(*sm, *vec, tau.reshape(1, N).expand(B, N).contiguous(), 0.99, stats=torch.full((8,), -2.0, device="cuda"))
    torch.cuda.synchronize()
    assert tuple(g_qr.shape) == (B, A, N) and tuple(g_iqn.shape) == (B, N, A)
    assert torch.equal(g_iqn.transpose(1, 2), g_qr)
    assert torch.equal(s_iqn, s_qr)


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("N", [1, 65, 200])
def test_quantile_act_and_iqn_act_are_one_algorithm(R, N):
    from jorldy_amd import ops

    A = 4
    rs = np.random.RandomState(100 * R + N)
    lg = cu(rs.randn(R, A, N).astype(np.float32))
    lg_sm = lg.transpose(1, 2).contiguous()
    eps = np.full(R, 0.5, np.float32)
    u = rs.rand(R)
    u[0] = 0.1  # at least one random row ...
    if R > 1:
        u[1] = 0.9  # ... and one greedy one
    ra = rs.randint(0, A, size=R).astype(np.int64)
    for draws in (dict(), dict(eps=eps, u=u, rand_action=ra)):
        a_qr, q_qr, all_qr = ops.quantile_act(lg, want_q_all=True, **draws)
        a_iqn, q_iqn, all_iqn = ops.iqn_act(lg_sm, want_q_all=True, **draws)
        torch.cuda.synchronize()
        assert torch.equal(a_iqn, a_qr) and torch.equal(q_iqn, q_qr) and torch.equal(all_iqn, all_qr)
        if draws:
            assert np.array_equal(npy(a_qr)[u < eps], ra[u < eps])


# ----------------------------------------------------------------------------------------------- the agent
def _agent_for(z, use_graph=True, lr=None, **over):
    from jorldy_amd.core.agent import Agent
    from test_agents_gpu import _h

    oc = {"name": "adam", "lr": _h(z, "lr") if lr is None else lr}
    if "hyper/optim_eps" in z.files and lr is None:
        oc["eps"] = _h(z, "optim_eps")
    kw = dict(state_size=int(_h(z, "S")), action_size=int(_h(z, "A")), hidden_size=int(_h(z, "H")), num_support=int(_h(z, "num_support")), optim_config=oc,
              gamma=_h(z, "gamma"), buffer_size=256, batch_size=int(_h(z, "B")), start_train_step=0, target_update_period=10000, run_step=100000, device="cuda",
              use_graph=use_graph)
    kw.update(over)
    return Agent("qrdqn", **kw)


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
def test_qrdqn_agent_learn_matches_reference(name):
    from oracle import synth
    from test_agents_gpu import _cmp_sd, _fill_from_fixture, _h, _sd
    from test_baseline_width_gpu import _thin_cmp

    z = load(name)
    agent = _agent_for(z)
    assert agent.backend == "native"
    assert np.array_equal(npy(agent.tau).reshape(-1), z["tau"])
    w0, wt = _initial_weights(z, agent)
    agent.network.load_state_dict(w0)
    agent.target_network.load_state_dict(wt)
    _fill_from_fixture(agent, z, False)
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    assert set(result) == {"loss", "epsilon", "max_Q", "max_logit", "min_logit"}
    for k in ("loss", "epsilon", "max_Q", "max_logit", "min_logit"):
        print(f"{name} result {k}: ours {result[k]!r} reference {float(z[f'result/{k}'])!r}")
        np.testing.assert_allclose(result[k], z[f"result/{k}"], rtol=1e-5, err_msg=k)
    B = int(_h(z, "B"))
    lg = npy(agent._static["logits"]).reshape(3, B, -1)
    for i, k in enumerate(("logit", "logit_next", "logit_target")):  # same sampled rows, same forwards
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


def test_qrdqn_graph_replay_equals_eager():
    """The assertions of test_td_agents_graph_replay_equals_eager, for QRDQN."""
    from test_agents_gpu import _fill_from_fixture, _sd

    z = load("qrdqn")
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


def test_q_network_with_3600_outputs_matches_float64():
    """18 actions x 200 quantiles: forward, backward and one Adam step of the q-network at the widest last layer a config asks for."""
    from test_rbnet_gpu import _force, _grads_vs_exact, _inputs, _mk_kind, _native_state

    S, A, H, B = 4, 3600, 64, 8
    (ref64, ref32), (tgt64, tgt32), nat = _mk_kind("q", "mlp", S, A, H, B)
    sd = nat.export_state()
    for k, v in ref32.state_dict().items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), k
    lr = 1e-3
    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    g = torch.Generator().manual_seed(1)
    for it in range(2):
        _force(nat, truth, lambda step: nat.set_hyper(lr, 0.9, 0.999, 1e-8, step), it)
        x_dev, x64 = _inputs("mlp", S, 2 * B, g)
        out = torch.empty(3, B, A, 1, device="cuda")
        nat.learn_forward(x_dev, B, None, out)
        x32 = x64.float()
        q0, q0_32 = ref64(x64[:B]), ref32(x32[:B])
        with torch.no_grad():
            q1, q1_32, q2, q2_32 = ref64(x64[B:]), ref32(x32[B:]), tgt64(x64[B:]), tgt32(x32[B:])
        T.vs_exact(out[0, :, :, 0], q0, q0_32, TOL, f"step {it} online(state)")
        T.vs_exact(out[1, :, :, 0], q1, q1_32, TOL, f"step {it} online(next_state)")
        T.vs_exact(out[2, :, :, 0], q2, q2_32, TOL, f"step {it} target(next_state)")
        gl = torch.randn(B, A, generator=g) / B
        truth.opt64.zero_grad()
        truth.opt32.zero_grad()
        q0.backward(gl.double())
        q0_32.backward(gl)
        nat.backward(gl.cuda().contiguous())
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"step {it} ")
        nat.optim_step("adam", None)
        truth.step(None, raw, *_native_state(nat), tag=f"adam step {it}")


def _act_agent(name, S, A, head, **extra):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    return Agent(name, state_size=S, action_size=A, hidden_size=64, head=head, optim_config={"name": "adam", "lr": 1e-4}, buffer_size=64, batch_size=8,
                 epsilon_init=0.5, device="cuda", **extra)


@pytest.mark.parametrize("head,S", [("mlp", 6), ("cnn", (4, 44, 52))])
def test_act_follows_the_reference_draw_order_and_takes_the_first_maximum_of_the_quantile_means(head, S):
    A, N, rows, steps = 3, 200, 2, 40
    agent = _act_agent("qrdqn", S, A, head, num_support=N)
    dqn = _act_agent("dqn", S, A, head)
    rs = np.random.RandomState(3)
    states = [rs.randint(0, 256, size=(rows,) + tuple(S), dtype=np.uint8) if head == "cnn" else rs.randn(rows, S).astype(np.float32) for _ in range(steps)]
    np.random.seed(5)
    ours = [agent.act(s, True)["action"] for s in states]
    np.random.seed(5)
    theirs = [dqn.act(s, True)["action"] for s in states]
    np.random.seed(5)
    n_rand = 0
    for s, a, a_dqn in zip(states, ours, theirs):
        assert a.shape == (rows, 1) and a.dtype == np.int64
        if np.random.random() < 0.5:  # qrdqn.py:38-42
            want = np.random.randint(0, A, size=(rows, 1))
            assert np.array_equal(a, want) and np.array_equal(a_dqn, want)
            n_rand += 1
        else:
            logits = agent.network(agent.as_tensor(s)).view(rows, A, N)
            q = logits.double().mean(-1).cpu().numpy()
            top = np.sort(q, -1)
            assert ((top[:, -1] - top[:, -2]) > 2.0 * N * 2.0 ** -24 * np.abs(npy(logits)).reshape(rows, -1).max(-1)).all(), "pick states without near-ties"
            assert np.array_equal(a.reshape(-1), q.argmax(-1))
            _, q32 = agent.logits2Q(logits)
            assert np.array_equal(a.reshape(-1), npy(torch.argmax(q32, -1)))
    assert 0 < n_rand < steps
    greedy = agent.act(states[0], False)["action"]  # epsilon_eval = 0: always the network
    logits = agent.network(agent.as_tensor(states[0])).view(rows, A, N)
    assert np.array_equal(greedy.reshape(-1), logits.double().mean(-1).cpu().numpy().argmax(-1))


QR_SUPPORTED = [
    ("config.qrdqn.cartpole", dict(state_size=4, action_size=2)),
    ("config.qrdqn.mountaincar", dict(state_size=2, action_size=3)),
    ("config.qrdqn.pong_mlagent", dict(state_size=8, action_size=3)),
    ("config.qrdqn.atari", dict(state_size=(4, 84, 84), action_size=6, head="cnn")),
    ("config.qrdqn.procgen", dict(state_size=(3, 64, 64), action_size=15, head="cnn")),
]


@pytest.mark.parametrize("label,kw", QR_SUPPORTED, ids=[c[0] for c in QR_SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(dict(hidden_size=64, optim_config={"name": "adam", "lr": 1e-4}, buffer_size=64, batch_size=8, device="cuda"), **kw)
    agent = Agent("qrdqn", **kw)
    assert agent.backend == "native" and agent.num_support == 200
    S = kw["state_size"]
    state = np.random.randint(0, 256, size=(2,) + tuple(S), dtype=np.uint8) if isinstance(S, tuple) else np.random.randn(2, S).astype(np.float32)
    for training in (True, False):  # epsilon 1: random; epsilon_eval 0: the network + jh_quantile_act
        a = agent.act(state, training)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))


def test_unsupported_configurations_raise_at_construction():
    from jorldy_amd.core.agent import Agent

    base = dict(state_size=4, action_size=2, hidden_size=64, optim_config={"name": "adam", "lr": 1e-4}, device="cuda")
    with pytest.raises(ValueError) as e:
        Agent("qrdqn", network="dueling", **base)
    assert "libjorldy_hip" in str(e.value) and "discrete_q_network" in str(e.value)
    with pytest.raises(ValueError) as e:
        Agent("qrdqn", num_support=98, **base)
    assert "98" in str(e.value)
    with pytest.raises(ValueError) as e:
        Agent("qrdqn", hidden_size=30, **{k: v for k, v in base.items() if k != "hidden_size"})
    assert "libjorldy_hip" in str(e.value)


def test_checkpoint_and_weight_sync_roundtrip(tmp_path):
    from test_agents_gpu import _fill_from_fixture, _sd

    z = load("qrdqn")
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
    for k in ("loss", "epsilon", "max_Q", "max_logit", "min_logit"):
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=1e-6, err_msg=k)
    flat = lambda ag: torch.cat([p.detach().reshape(-1) for p in ag.network.parameters()])
    torch.testing.assert_close(flat(b), flat(a), rtol=1e-5, atol=1e-6)
    c = _agent_for(z)
    c.sync_in(a.sync_out()["weights"])
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, c.network.state_dict()[k]), k


# ----------------------------------------------------------------------------------------------- learning curve
CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, hidden=512, batch=32, num_support=200, lr=1e-4, eps=1e-2 / 32, gamma=0.99,
                    epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


def test_qrdqn_cartpole_learning_curve_tracks_the_reference():
    """config.qrdqn.cartpole in the single-mode loop of test_learning_curve_gpu._dqn_curve, three seeds, next to the curve of the REAL
    reference agent on the oracle's bit-identical CartPole (tests/golden/curves_reference_qrdqn.json, tools/gen_golden_qrdqn.py).  The
    assertions are the DQN curve test's: both start near random play, both learn, and the ends lie within a factor 2 of each other."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from test_learning_curve_gpu import DQN_CHUNK, DQN_RUN_STEP, DQN_STEPS, _dqn_curve

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curves_reference_qrdqn.json")) as f:
        fx = json.load(f)
    c = CURVE_CONFIG
    assert fx["qrdqn_cartpole"]["config"] == c
    assert (c["steps"], c["run_step"], c["chunk"]) == (DQN_STEPS, DQN_RUN_STEP, DQN_CHUNK)
    ref = fx["qrdqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == DQN_STEPS // DQN_CHUNK for r in ref)

    def gpu_env(seed):
        env = ops.CartPoleVec(1, seed=1000 + seed)
        return env, env.obs().copy()

    def gpu_step(env, action):
        nxt, rew, done = env.step(action)
        return nxt.copy(), rew.reshape(1, 1).astype(np.float64), done.reshape(1, 1).astype(bool), env.obs().copy()

    make = lambda: Agent("qrdqn", state_size=4, action_size=2, hidden_size=c["hidden"], network="discrete_q_network", num_support=c["num_support"],
                         optim_config={"name": "adam", "lr": c["lr"], "eps": c["eps"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"],
                         epsilon_min=c["epsilon_min"], explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"],
                         start_train_step=c["start"], target_update_period=c["target"], lr_decay=c["lr_decay"], run_step=c["run_step"], device="cuda")
    gpu = [_dqn_curve(make, gpu_env, gpu_step, s) for s in (1, 2, 3)]
    print(json.dumps({"steps": DQN_STEPS, "chunk": DQN_CHUNK, "metric": "mean episode length per 1000 env steps (max 500)", "hip": gpu, "reference": ref}))
    g_start, g_end = np.mean([np.mean(x[:2]) for x in gpu]), np.mean([np.mean(x[-4:]) for x in gpu])
    c_start, c_end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    print(f"QR-DQN episode length: HIP {g_start:.1f} -> {g_end:.1f}, reference {c_start:.1f} -> {c_end:.1f}")
    assert g_start < 40 and c_start < 40  # random policy: ~22 steps
    assert g_end > 4 * g_start and c_end > 4 * c_start  # both learn
    assert 0.5 * c_end <= g_end <= 2.0 * c_end
