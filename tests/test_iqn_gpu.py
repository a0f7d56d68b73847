"""IQN on the GPU: the kernels of jh_iqn.hip (cosine features, Hadamard product and its backward, jh_iqn_loss, jh_iqn_act) and the
network object (ops.IQNNet) against the float64 truth of tests/iqn_truth.py (pinned to the reference's own learn() by
tests/test_iqn_cpu.py) and against the fixtures of tools/gen_golden_iqn.py; then the whole agent: one learn() per fixture with the
fixture's tau draws injected, hipGraph replay against eager, acting in the reference's draw order with the training / evaluation tau
ranges, the configs' shapes, checkpoints, and the learning curve of config.iqn.cartpole next to the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import iqn_truth as I
import margins
from oracle import synth
from tests.util import cu, f32, load, npy

pytestmark = pytest.mark.gpu

FIXTURES = ["iqn", "iqn_odd", "iqn_cartpole"]
TOL = 1e-5


# ----------------------------------------------------------------------------------------------- elementwise kernels
@pytest.mark.parametrize("E", [1, 4, 10, 64])
def test_cosine_features_match_float64_on_the_float32_argument(E):
    from jorldy_amd import ops

    rs = np.random.RandomState(E)
    tau = np.concatenate([np.array([0.0, 1.0, 2.0 ** -24, 0.5], dtype=np.float32), rs.rand(1021).astype(np.float32)])  # 1025 rows: more than one block
    ours = ops.iqn_cos_features(f32(tau), E)
    torch.cuda.synchronize()
    assert tuple(ours.shape) == (tau.size, E)
    e = T.vs_exact(ours, I.cos_features(tau, E, torch.float64), I.cos_features(tau, E, torch.float32), TOL, f"cos features E={E}")
    print(f"E={E}: |ours - fp64| = {e[0]:.3e} (torch-cpu-fp32: {e[1]:.3e})")
    assert np.array_equal(npy(ours)[0], np.ones(E, np.float32))  # tau = 0
    shaped = ops.iqn_cos_features(f32(tau[:1024].reshape(4, 256)), E)
    assert tuple(shaped.shape) == (4, 256, E) and torch.equal(shaped.reshape(1024, E), ours[:1024])


@pytest.mark.parametrize("B,N,H", [(1, 1, 4), (2, 256, 8), (7, 33, 64), (3, 5, 512)])
def test_hadamard_product_and_its_backward_match_float64(B, N, H):
    from jorldy_amd import ops

    rs = np.random.RandomState(B * 1000 + N + H)
    psi_pre, phi_pre, g = rs.randn(B, H).astype(np.float32), rs.randn(B, N, H).astype(np.float32), rs.randn(B, N, H).astype(np.float32)
    psi, phi = np.maximum(psi_pre, 0), np.maximum(phi_pre, 0)
    emb = ops.iqn_hadamard(f32(psi), f32(phi))
    assert np.array_equal(npy(emb), psi[:, None, :] * phi)  # one float32 product per element
    dphi, dpsi = ops.iqn_hadamard_backward(f32(g), f32(psi), f32(phi))
    torch.cuda.synchronize()
    dpsi64, dphi64 = I.hadamard_backward(psi_pre, phi_pre, g, torch.float64)
    dpsi32, dphi32 = I.hadamard_backward(psi_pre, phi_pre, g, torch.float32)
    T.vs_exact(dphi, dphi64, dphi32, TOL, f"d(phi_pre) B{B} N{N} H{H}")
    e = T.vs_exact(dpsi, dpsi64, dpsi32, TOL, f"d(psi_pre) B{B} N{N} H{H}")
    print(f"B{B} N{N} H{H}: d(psi_pre) |ours - fp64| = {e[0]:.3e} (torch-cpu-fp32: {e[1]:.3e})")
    assert not npy(dphi)[phi_pre <= 0].any() and not npy(dpsi)[psi_pre <= 0].any()
    for _ in range(2):  # the sum over n runs in a fixed order
        dphi2, dpsi2 = ops.iqn_hadamard_backward(f32(g), f32(psi), f32(phi))
        assert torch.equal(dphi, dphi2) and torch.equal(dpsi, dpsi2)


# ----------------------------------------------------------------------------------------------- the loss kernel
def _fixture_inputs(z):
    d = {k: z[f"learn/{s}"] for k, s in (("logit", "logit"), ("next_online", "logit_next"), ("target", "logit_target"))}
    d.update({k: z[f"learn/{k}"].reshape(-1) for k in ("action", "reward", "done")})
    d["tau"] = z["learn/tau"][0]
    return d


def _run_kernel(d, gamma, stats=None):
    from jorldy_amd import ops

    g, st = ops.iqn_loss(f32(d["logit"]), f32(d["next_online"]), f32(d["target"]), f32(d["action"]), f32(d["reward"]), f32(d["done"]), f32(d["tau"]), gamma, stats=stats)
    torch.cuda.synchronize()
    return npy(g), npy(st)


def _truth_following_near_ties(d, gamma, grad):
    """tests/test_qrdqn_gpu.py's rule: on rows whose two best means of online(s') are closer than two fp32 sums of N terms can be off
    by, either of the two is a correct selection and the truth takes the one the kernel's gradient shows.  -> (truth, number of such rows)."""
    t = I.iqn_loss(gamma=gamma, **d)
    near = np.nonzero(t["gap"] <= t["gap_bound"])[0]
    if near.size == 0:
        return t, 0
    qn = np.asarray(d["next_online"], dtype=np.float64).mean(1)
    alt = t["a_star"].copy()
    alt[near] = np.argsort(-qn[near], axis=-1, kind="stable")[:, 1]
    t_alt = I.iqn_loss(gamma=gamma, a_star=alt, **d)
    pick = t["a_star"].copy()
    for b in near:
        if np.abs(grad[b] - t_alt["grad"][b]).max() < np.abs(grad[b] - t["grad"][b]).max():
            pick[b] = alt[b]
    return I.iqn_loss(gamma=gamma, a_star=pick, **d), int(near.size)


def _check_stats(st, want, what):
    for i, k in enumerate(("loss", "max_Q", "max_logit", "min_logit")):
        print(f"{what} {k}: ours {st[i]!r} want {want[k]!r}")
        np.testing.assert_allclose(st[i], want[k], rtol=1e-5, err_msg=f"{what} {k}")
    assert st[4] == 0.0 and st[5] == 0.0 and st[6] == 0.0 and st[7] == 0.0


def _others_are_zero(grad, action):
    B, N, A = grad.shape
    act = np.clip(np.asarray(action).astype(np.int64), 0, A - 1)
    other = np.ones((B, N, A), bool)
    other[np.arange(B), :, act] = False
    assert not grad[other].any(), "the entries of the actions not taken must be written as zeros"


@pytest.mark.parametrize("name", FIXTURES)
def test_iqn_loss_matches_the_reference_fixture(name):
    z = load(name)
    d = _fixture_inputs(z)
    gamma = float(z["hyper/gamma"])
    grad, st = _run_kernel(d, gamma, stats=torch.full((8,), -1.0, device="cuda"))
    _check_stats(st, {k: float(z[f"result/{k}"]) for k in ("loss", "max_Q", "max_logit", "min_logit")}, name)
    t, near = _truth_following_near_ties(d, gamma, grad)
    assert near == 0
    assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(-1))
    e = T.grad_vs_exact(grad, t["grad"], z["learn/d_logit"], TOL, f"{name} d(loss)/d(logit)")
    print(f"{name}: gradient |ours - fp64| / max = {e[0]:.3e} (reference fp32: {e[1]:.3e})")
    _others_are_zero(grad, d["action"])


@pytest.mark.parametrize("B,A,N,variant", I.SWEEP, ids=[f"B{c[0]}-A{c[1]}-N{c[2]}-{c[3]}" for c in I.SWEEP])
def test_iqn_loss_matches_float64_truth_over_a_sweep(B, A, N, variant):
    d = I.sweep_case(B, A, N, variant)
    grad, st = _run_kernel(d, 0.99, stats=torch.full((8,), -1.0, device="cuda"))
    t, near = _truth_following_near_ties(d, 0.99, grad)
    print(f"rows with a near-tie of the two best next actions: {near} of {B}")
    assert near <= 0.01 * B
    _check_stats(st, t, f"B{B} A{A} N{N} {variant}")
    t32 = I.iqn_loss(gamma=0.99, dtype=torch.float32, a_star=t["a_star"] if near == 0 else None, **d)
    e = T.grad_vs_exact(grad, t["grad"], t32["grad"] if near == 0 else None, TOL, "d(loss)/d(logit)")
    print(f"gradient |ours - fp64| / max = {e[0]:.3e}")
    _others_are_zero(grad, d["action"])


def test_iqn_loss_is_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B, A, N in ((32, 2, 64), (255, 6, 51), (7, 5, 33)):
        d = I.sweep_case(B, A, N, "plain", seed=1)
        args = [f32(d[k]) for k in ("logit", "next_online", "target", "action", "reward", "done", "tau")]
        g1, s1 = ops.iqn_loss(*args, 0.99)
        g2, s2 = ops.iqn_loss(*args, 0.99)
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(s1, s2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            g3, s3 = ops.iqn_loss(*args, 0.99)
        g3.fill_(7.0)
        s3.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, g3) and torch.equal(s1, s3)


@pytest.mark.parametrize("N", [0, 257])
def test_iqn_loss_rejects_out_of_range_sizes(N):
    from jorldy_amd import _lib, ops

    z = torch.zeros(2, N, 2, device="cuda")
    v = torch.zeros(2, device="cuda")
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.iqn_loss(z, z, z, v, v, v, torch.zeros(2, N, device="cuda"), 0.99)


# ----------------------------------------------------------------------------------------------- the acting kernel
@pytest.mark.parametrize("R", [1, 5, 64])
@pytest.mark.parametrize("N", [1, 64])
def test_iqn_act_matches_numpy(R, N):
    from jorldy_amd import ops

    A = 4
    rs = np.random.RandomState(100 * R + N)
    lg = rs.randn(R, N, A).astype(np.float32)
    lg[0, :, 1] = lg[0, :, 3] = np.abs(lg[0]).max(-1) + 1.0  # two identical columns that are the maximum: the first one wins
    if R > 2:
        lg[2, :, 0] = lg[2, :, 2] = np.abs(lg[2]).max(-1) + 1.0
    q64 = lg.astype(np.float64).mean(1)
    top = np.sort(q64, -1)
    clear = (top[:, -1] - top[:, -2]) > 2.0 * N * 2.0 ** -24 * np.abs(lg).reshape(R, -1).max(-1)
    clear[0] = True  # exact ties: identical columns give identical sums
    if R > 2:
        clear[2] = True
    assert clear.all()
    want = q64.argmax(-1)
    assert want[0] == 1 and (R <= 2 or want[2] == 0)
    act, q, q_all = ops.iqn_act(cu(lg), want_q_all=True)
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
    act2, q2, _ = ops.iqn_act(cu(lg), eps=eps, u=u, rand_action=ra)
    torch.cuda.synchronize()
    taken = np.where(u < eps, ra, want)
    assert np.array_equal(npy(act2), taken)
    assert np.array_equal(npy(q2), npy(q_all)[np.arange(R), taken])
    out = (torch.full((R,), -1, dtype=torch.int64, device="cuda"), torch.zeros(R, device="cuda"))
    ops.iqn_act(cu(lg), out=out)
    torch.cuda.synchronize()
    assert np.array_equal(npy(out[0]), want)


# ----------------------------------------------------------------------------------------------- the network object
def _mirror64(S, A, E, N, H, seed):
    from jorldy_amd.core.network import Network

    torch.manual_seed(seed)
    m = Network("iqn", S, A, E, N, D_hidden=H).double()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))  # biases away from their zero initialisation
    T.round_to_fp32_(m)
    return m, T.as32(m)


def _fwd(mod, x, tau):
    return I.iqn_forward(dict(mod.named_parameters()), x, tau, next(mod.parameters()).dtype)


@pytest.mark.parametrize("S,A,H,E,N,B", I.NET_SHAPES)
def test_iqnnet_three_forwards_backward_and_adam_match_float64(S, A, H, E, N, B):
    """learn_forward, backward and two teacher-forced Adam steps of ops.IQNNet against float64 (as test_q_network_with_3600_outputs_matches_float64)."""
    from jorldy_amd import ops
    from test_rbnet_gpu import _force, _grads_vs_exact, _native_state

    ref64, ref32 = _mirror64(S, A, E, N, H, 0)
    tgt64, tgt32 = _mirror64(S, A, E, N, H, 100)
    nat = ops.IQNNet(S, A, E, N, H, B, "cuda:0")
    assert (nat.maxB, nat.A, nat.K, nat.cnn, nat.noise_len, nat.kind) == (B, A, N, False, 0, "iqn")
    nat.import_state(ref32.state_dict(), nat.params)
    nat.import_state(tgt32.state_dict(), nat.target)
    sd = nat.export_state()
    assert list(sd.keys()) == list(ref32.state_dict().keys()) == list(I.KEYS)
    for k, v in ref32.state_dict().items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), k
    lr = 1e-3
    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    g = torch.Generator().manual_seed(1)
    for it in range(2):
        _force(nat, truth, lambda step: nat.set_hyper(lr, 0.9, 0.999, 1e-8, step), it)
        x = torch.randn(2 * B, S, generator=g)
        tau = torch.rand(3, B, N, generator=g)
        x_dev, tau_dev = x.cuda(), tau.cuda()
        out = torch.empty(3, B, N, A, device="cuda")
        nat.learn_forward(x_dev, B, tau_dev, out)
        tn = tau.numpy()
        q0, q0_32 = _fwd(ref64, x[:B], tn[0]), _fwd(ref32, x[:B], tn[0])
        with torch.no_grad():
            q1, q1_32, q2, q2_32 = _fwd(ref64, x[B:], tn[1]), _fwd(ref32, x[B:], tn[1]), _fwd(tgt64, x[B:], tn[2]), _fwd(tgt32, x[B:], tn[2])
        T.vs_exact(out[0], q0, q0_32, TOL, f"step {it} online(state)")
        T.vs_exact(out[1], q1, q1_32, TOL, f"step {it} online(next_state)")
        T.vs_exact(out[2], q2, q2_32, TOL, f"step {it} target(next_state)")
        if it == 0:  # the acting forward gives the same values (and does not disturb what backward needs when it runs first)
            single = nat.forward(x_dev[B:], 1, tau_dev[2])
            T.vs_exact(single, q2, q2_32, TOL, "forward(target, next_state)")
            nat.learn_forward(x_dev, B, tau_dev, out)
        gl = torch.randn(B, N, A, generator=g) / (B * N)
        truth.opt64.zero_grad()
        truth.opt32.zero_grad()
        q0.backward(gl.double())
        q0_32.backward(gl)
        nat.backward(gl.cuda().contiguous())
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"step {it} ")
        nat.optim_step("adam", None)
        truth.step(None, raw, *_native_state(nat), tag=f"adam step {it}")
    with pytest.raises(ValueError):
        nat.optim_step("rmsprop", None)


# ----------------------------------------------------------------------------------------------- the agent
def _agent_for(z, use_graph=True, lr=None, **over):
    from jorldy_amd.core.agent import Agent
    from test_agents_gpu import _h

    oc = {"name": "adam", "lr": _h(z, "lr") if lr is None else lr}
    if "hyper/optim_eps" in z.files and lr is None:
        oc["eps"] = _h(z, "optim_eps")
    kw = dict(state_size=int(_h(z, "S")), action_size=int(_h(z, "A")), num_sample=int(_h(z, "N")), embedding_dim=int(_h(z, "E")), optim_config=oc,
              gamma=_h(z, "gamma"), buffer_size=256, batch_size=int(_h(z, "B")), start_train_step=0, target_update_period=10000, run_step=100000, device="cuda",
              use_graph=use_graph)
    kw.update(over)
    return Agent("iqn", **kw)


def _initial_weights(z, agent):
    shapes = {k: v.shape for k, v in agent.network.state_dict().items()}
    assert [(k, tuple(int(x) for x in z[f"shape/{k}"])) for k in shapes] == [(k, tuple(v)) for k, v in shapes.items()]
    seed = int(z["recipe_seed"])
    return ({k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed).items()},
            {k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed + 1).items()})


def _thin_cmp(ours, z, prefix, scale_of=None, tol=1e-5, what="", only_stored=False):
    """test_baseline_width_gpu._thin_cmp with the fixture's own thinning stride."""
    stride = int(z["thin_stride"])
    for k, v in ours.items():
        if only_stored and prefix + k not in z.files:
            continue
        ref = z[prefix + k]
        got = synth.thin(np.asarray(v), stride=stride)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        scale = float(scale_of(k)) if scale_of else float(np.abs(ref).max())
        err = float(np.abs(got - ref).max()) / (scale + 1e-30)
        margins.leq(err, tol, f"{what} {k}: max |diff| / the tensor's largest entry")


def _loaded_agent(z, **kw):
    from test_agents_gpu import _fill_from_fixture

    agent = _agent_for(z, **kw)
    w0, wt = _initial_weights(z, agent)
    agent.network.load_state_dict(w0)
    agent.target_network.load_state_dict(wt)
    _fill_from_fixture(agent, z, False)
    return agent, w0, wt


@pytest.mark.parametrize("name", FIXTURES)
def test_iqn_agent_learn_matches_reference(name):
    """The assertions and caps of test_qrdqn_agent_learn_matches_reference, with the fixture's three tau draws injected."""
    from test_agents_gpu import _h

    z = load(name)
    agent, w0, wt = _loaded_agent(z)
    assert agent.backend == "native" and agent._net.H == 512 and agent._net.kind == "iqn"
    agent._tau_inject = z["learn/tau"]
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    assert set(result) == {"loss", "epsilon", "max_Q", "max_logit", "min_logit"}
    for k in ("loss", "epsilon", "max_Q", "max_logit", "min_logit"):
        print(f"{name} result {k}: ours {result[k]!r} reference {float(z[f'result/{k}'])!r}")
        np.testing.assert_allclose(result[k], z[f"result/{k}"], rtol=1e-5, err_msg=k)
    lg = npy(agent._static["logits"])
    for i, k in enumerate(("logit", "logit_next", "logit_target")):  # same sampled rows, same draws, same forwards
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


def test_iqn_graph_replay_equals_eager():
    """The assertions of test_td_agents_graph_replay_equals_eager, for IQN: the tau draws are made eagerly in front of every replay."""
    z = load("iqn")
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
    """Learning rate 0 and the same sampled rows: two consecutive replays differ only in their tau draws -- and so does the loss; with
    the draws injected they give the same bits."""
    z = load("iqn")
    torch.manual_seed(0)
    agent, _, _ = _loaded_agent(z, lr=0.0, lr_decay=False)
    losses = []
    for it in range(4):
        np.random.seed(7)
        losses.append(agent.learn()["loss"])
    assert agent._graph is not None
    assert losses[2] != losses[3] and len(set(losses)) == 4
    agent._tau_inject = z["learn/tau"]
    fixed = []
    for it in range(2):
        np.random.seed(7)
        fixed.append(agent.learn()["loss"])
    assert fixed[0] == fixed[1] and fixed[0] not in losses


def _act_agent(name, S, A, **extra):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    return Agent(name, state_size=S, action_size=A, optim_config={"name": "adam", "lr": 1e-4}, buffer_size=64, batch_size=8, epsilon_init=0.5, device="cuda", **extra)


def _truth_actions(agent, states, tau):
    sd = {k: v.cpu() for k, v in agent.network.state_dict().items()}
    with torch.no_grad():
        logits = I.iqn_forward(sd, states, tau)
    q = logits.mean(1).numpy()
    top = np.sort(q, -1)
    N = logits.shape[1]
    assert ((top[:, -1] - top[:, -2]) > 2.0 * N * 2.0 ** -24 * np.abs(logits.numpy()).reshape(q.shape[0], -1).max(-1)).all(), "pick states without near-ties"
    return q.argmax(-1)


def test_act_follows_the_reference_draw_order_and_the_tau_ranges():
    S, A, N, rows, steps = 6, 3, 16, 2, 40
    agent = _act_agent("iqn", S, A, num_sample=N, embedding_dim=8, sample_min=0.25, sample_max=0.25)
    dqn = _act_agent("dqn", S, A, hidden_size=64)
    rs = np.random.RandomState(3)
    states = [rs.randn(rows, S).astype(np.float32) for _ in range(steps)]
    tau_fixed = rs.rand(rows, N).astype(np.float32)
    agent._tau_inject = tau_fixed
    np.random.seed(5)
    ours = [agent.act(s, True)["action"] for s in states]
    np.random.seed(5)
    theirs = [dqn.act(s, True)["action"] for s in states]
    np.random.seed(5)
    n_rand = 0
    for s, a, a_dqn in zip(states, ours, theirs):
        assert a.shape == (rows, 1) and a.dtype == np.int64
        if np.random.random() < 0.5:  # iqn.py:67-71
            want = np.random.randint(0, A, size=(rows, 1))
            assert np.array_equal(a, want) and np.array_equal(a_dqn, want)
            n_rand += 1
        else:
            assert np.array_equal(a.reshape(-1), _truth_actions(agent, s, tau_fixed))
    assert 0 < n_rand < steps
    # the ranges of the draws themselves: [0, 1] when training, [sample_min, sample_max] otherwise (iqn.py:64-65)
    agent._tau_inject = None
    seen = []
    inner = agent._net.draw_tau
    agent._net.draw_tau = lambda *a, **k: seen.append(inner(*a, **k)) or seen[-1]
    agent.epsilon = 0.0
    big = rs.randn(8, S).astype(np.float32)
    agent.act(big, True)
    t = npy(seen[-1])
    assert t.shape == (8, N) and 0.0 <= t.min() < 0.2 and 0.8 < t.max() <= 1.0
    greedy = agent.act(big, False)["action"]  # epsilon_eval = 0: always the network, at tau = 0.25
    assert np.array_equal(npy(seen[-1]), np.full((8, N), 0.25, np.float32))
    assert np.array_equal(greedy.reshape(-1), _truth_actions(agent, big, np.full((8, N), 0.25, np.float32)))
    # agent.network is called as the reference's module is
    logits, tau = agent.network(agent.as_tensor(big), 0.25, 0.25)
    assert tuple(logits.shape) == (8, N, A) and tuple(tau.shape) == (8, N, 1) and bool((tau == 0.25).all())
    _, q = agent.logits2Q(logits)
    assert np.array_equal(npy(torch.argmax(q, -1)), greedy.reshape(-1))


IQN_SUPPORTED = [
    ("config.iqn.cartpole", dict(state_size=4, action_size=2)),
    ("config.iqn.mountaincar", dict(state_size=2, action_size=3)),
    ("config.iqn.pong_mlagent", dict(state_size=8, action_size=3)),
]


@pytest.mark.parametrize("label,kw", IQN_SUPPORTED, ids=[c[0] for c in IQN_SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(dict(network="iqn", optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}, buffer_size=64, batch_size=32, num_sample=64, embedding_dim=64,
                   sample_min=0.0, sample_max=1.0, device="cuda"), **kw)
    agent = Agent("iqn", **kw)
    assert agent.backend == "native" and agent.num_support == 64 and agent._net.H == 512
    S = kw["state_size"]
    state = np.random.randn(2, S).astype(np.float32)
    for training in (True, False):  # epsilon 1: random; epsilon_eval 0: the network + jh_iqn_act
        a = agent.act(state, training)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))


def test_unsupported_configurations_raise_at_construction():
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.iqn import IQN_ELIGIBLE

    base = dict(state_size=4, action_size=2, optim_config={"name": "adam", "lr": 1e-4}, device="cuda")
    for over in (dict(head="cnn", state_size=(4, 84, 84)), dict(state_size=(4,)), dict(network="discrete_q_network"), dict(optim_config={"name": "rmsprop", "lr": 1e-4}),
                 dict(num_sample=0), dict(num_sample=257), dict(sample_min=0.5, sample_max=0.25), dict(sample_max=1.01), dict(sample_min=-0.01)):
        with pytest.raises(ValueError) as e:
            Agent("iqn", **dict(base, **over))
        assert IQN_ELIGIBLE in str(e.value), over


def test_checkpoint_and_weight_sync_roundtrip(tmp_path):
    z = load("iqn")
    a, _, _ = _loaded_agent(z)
    np.random.seed(3)
    a.learn()  # the checkpoint carries Adam moments and a step count
    a.update_target()  # load() gives both networks the checkpoint's weights (dqn.py:190-199)
    a.save(str(tmp_path))
    # the reference's format: torch.optim.Adam over the reference-shaped parameters takes the optimizer state
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert list(ckpt["network"].keys()) == list(I.KEYS)
    params = [torch.nn.Parameter(v.clone()) for v in ckpt["network"].values()]
    opt = torch.optim.Adam(params, lr=1e-3)
    opt.load_state_dict(ckpt["optimizer"])
    for p in params:
        assert opt.state[p]["exp_avg"].shape == p.shape and opt.state[p]["exp_avg_sq"].shape == p.shape and float(opt.state[p]["step"]) == 1.0
    from test_agents_gpu import _fill_from_fixture

    b = _agent_for(z)
    b.load(str(tmp_path))
    _fill_from_fixture(b, z, False)
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, b.network.state_dict()[k]) and torch.equal(v, b.target_network.state_dict()[k]), k
    res = []
    for ag in (a, b):
        np.random.seed(11)
        ag._tau_inject = z["learn/tau"]
        res.append(ag.learn())
        ag._tau_inject = None
    for k in ("loss", "epsilon", "max_Q", "max_logit", "min_logit"):
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


# ----------------------------------------------------------------------------------------------- learning curve
CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, batch=32, num_sample=64, embedding_dim=64, sample_min=0.0, sample_max=1.0,
                    lr=1e-4, eps=1e-2 / 32, gamma=0.99, epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


def test_iqn_cartpole_learning_curve_tracks_the_reference():
    """config.iqn.cartpole in the single-mode loop of test_learning_curve_gpu._dqn_curve, three seeds, next to the curve of the REAL
    reference agent on the oracle's bit-identical CartPole (tests/golden/curves_reference_iqn.json, tools/gen_golden_iqn.py).  The
    assertions are the QR-DQN curve test's: both start near random play, both learn, and the ends lie within a factor 2 of each other."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from test_learning_curve_gpu import DQN_CHUNK, DQN_RUN_STEP, DQN_STEPS, _dqn_curve

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curves_reference_iqn.json")) as f:
        fx = json.load(f)
    c = CURVE_CONFIG
    assert fx["iqn_cartpole"]["config"] == c
    assert (c["steps"], c["run_step"], c["chunk"]) == (DQN_STEPS, DQN_RUN_STEP, DQN_CHUNK)
    ref = fx["iqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == DQN_STEPS // DQN_CHUNK for r in ref)

    def gpu_env(seed):
        env = ops.CartPoleVec(1, seed=1000 + seed)
        return env, env.obs().copy()

    def gpu_step(env, action):
        nxt, rew, done = env.step(action)
        return nxt.copy(), rew.reshape(1, 1).astype(np.float64), done.reshape(1, 1).astype(bool), env.obs().copy()

    make = lambda: Agent("iqn", state_size=4, action_size=2, network="iqn", num_sample=c["num_sample"], embedding_dim=c["embedding_dim"], sample_min=c["sample_min"],
                         sample_max=c["sample_max"], optim_config={"name": "adam", "lr": c["lr"], "eps": c["eps"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"],
                         epsilon_min=c["epsilon_min"], explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"],
                         start_train_step=c["start"], target_update_period=c["target"], lr_decay=c["lr_decay"], run_step=c["run_step"], device="cuda")
    gpu = [_dqn_curve(make, gpu_env, gpu_step, s) for s in (1, 2, 3)]
    print(json.dumps({"steps": DQN_STEPS, "chunk": DQN_CHUNK, "metric": "mean episode length per 1000 env steps (max 500)", "hip": gpu, "reference": ref}))
    g_start, g_end = np.mean([np.mean(x[:2]) for x in gpu]), np.mean([np.mean(x[-4:]) for x in gpu])
    c_start, c_end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    print(f"IQN episode length: HIP {g_start:.1f} -> {g_end:.1f}, reference {c_start:.1f} -> {c_end:.1f}")
    assert g_start < 40 and c_start < 40  # random policy: ~22 steps
    assert g_end > 4 * g_start and c_end > 4 * c_start  # both learn
    assert 0.5 * c_end <= g_end <= 2.0 * c_end
