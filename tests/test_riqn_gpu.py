"""Rainbow-IQN on the GPU: jh_riqn_loss (the quantile family's kernel under the n-step return, the importance weights and the priorities) and
the network object (ops.RainbowIQNNet: IQN's trunk under Rainbow's noisy dueling tail) against the float64 truth of tests/riqn_truth.py
(pinned to the reference's own learn() by tests/test_riqn_cpu.py); then the whole agent against the fixtures of tools/gen_golden_riqn.py
with the recorded tau and noise draws injected, hipGraph replay against eager, acting, checkpoints, the configs' shapes and the learning
curve of the reduced config.rainbow_iqn.cartpole next to the reference's."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import iqn_truth as I
import margins
import riqn_truth as R
from oracle import synth
from tests.util import cu, f32, load, npy

pytestmark = pytest.mark.gpu

FIXTURES = ["riqn", "riqn_odd", "riqn_cartpole"]
TOL = 1e-5


# ----------------------------------------------------------------------------------------------- the loss kernel
def _run_kernel(d, gamma, alpha, n_step, stats=None):
    from jorldy_amd import ops

    g, prio, st = ops.riqn_loss(f32(d["logit"]), f32(d["next_online"]), f32(d["target"]), f32(d["action"]), f32(d["reward"]), f32(d["done"]), f32(d["weights"]),
                                f32(d["tau"]), gamma, alpha, n_step, stats=stats)
    torch.cuda.synchronize()
    return npy(g), npy(prio), npy(st)


def _others_are_zero(grad, action):
    B, N, A = grad.shape
    act = np.clip(np.asarray(action).astype(np.int64), 0, A - 1)
    other = np.ones((B, N, A), bool)
    other[np.arange(B), :, act] = False
    assert not grad[other].any(), "the entries of the actions not taken must be written as zeros"


@pytest.mark.parametrize("B,A,N,n_step", R.SWEEP, ids=[f"B{c[0]}-A{c[1]}-N{c[2]}-n{c[3]}" for c in R.SWEEP])
def test_riqn_loss_matches_float64_truth_over_a_sweep(B, A, N, n_step):
    """Gradient, priorities and statistics; tests/test_riqn_cpu.py proves that no row of a case sits on a near-tie of the selection or
    within 2^-20 of a kink, so the truth's own selection holds for every row and no case passes a_star."""
    d, _ = R.sweep_case(B, A, N, n_step)
    grad, prio, st = _run_kernel(d, R.SWEEP_GAMMA, R.SWEEP_ALPHA, n_step, stats=torch.full((8,), -1.0, device="cuda"))
    t = R.riqn_loss(gamma=R.SWEEP_GAMMA, alpha=R.SWEEP_ALPHA, **d)
    t32 = R.riqn_loss(gamma=R.SWEEP_GAMMA, alpha=R.SWEEP_ALPHA, dtype=torch.float32, **d)
    assert np.array_equal(t["a_star"], t32["a_star"])
    for i, k in enumerate(("loss", "max_Q", "max_logit", "min_logit")):
        print(f"{k}: ours {st[i]!r} want {t[k]!r}")
        np.testing.assert_allclose(st[i], t[k], rtol=1e-5, err_msg=k)
    assert st[4] == 0.0 and st[5] == 0.0 and st[6] == 0.0 and st[7] == 0.0
    e = T.grad_vs_exact(grad, t["grad"], t32["grad"], TOL, "d(loss)/d(logit)")
    print(f"gradient |ours - fp64| / max = {e[0]:.3e} (torch-cpu-fp32: {e[1]:.3e})")
    e = T.grad_vs_exact(prio, t["prio"], t32["prio"], TOL, "priorities")
    print(f"priorities |ours - fp64| / max = {e[0]:.3e} (torch-cpu-fp32: {e[1]:.3e})")
    _others_are_zero(grad, d["action"])


@pytest.mark.parametrize("B,A,N", I.SWEEP_SHAPES)
def test_riqn_loss_with_one_step_and_unit_weights_is_iqn_loss_bit_for_bit(B, A, N):
    from jorldy_amd import ops

    for variant in I.VARIANTS:
        d = I.sweep_case(B, A, N, variant)
        args = [f32(d[k]) for k in ("logit", "next_online", "target", "action", "reward", "done")]
        g0, s0 = ops.iqn_loss(*args, f32(d["tau"]), 0.99)
        ones = torch.ones(B, device="cuda")
        for n_step in (0, 1):
            g1, prio, s1 = ops.riqn_loss(*args, ones, f32(d["tau"]), 0.99, 0.6, n_step)
            torch.cuda.synchronize()
            assert torch.equal(g0, g1) and torch.equal(s0, s1), (variant, n_step)
        t = R.riqn_loss(d["logit"], d["next_online"], d["target"], d["action"], d["reward"].reshape(B, 1), d["done"].reshape(B, 1), np.ones(B, np.float32), d["tau"], 0.99, 0.6)
        np.testing.assert_allclose(npy(prio), t["prio"], rtol=1e-5)


def test_riqn_loss_is_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B, A, N, n_step in ((3, 5, 63, 2), (257, 2, 65, 5), (3, 64, 256, 1)):
        d, _ = R.sweep_case(B, A, N, n_step)
        args = [f32(d[k]) for k in ("logit", "next_online", "target", "action", "reward", "done", "weights", "tau")]
        g1, p1, s1 = ops.riqn_loss(*args, 0.99, 0.6, n_step)
        g2, p2, s2 = ops.riqn_loss(*args, 0.99, 0.6, n_step)
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(p1, p2) and torch.equal(s1, s2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            g3, p3, s3 = ops.riqn_loss(*args, 0.99, 0.6, n_step)
        g3.fill_(7.0)
        p3.fill_(7.0)
        s3.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, g3) and torch.equal(p1, p3) and torch.equal(s1, s3)


@pytest.mark.parametrize("N,n_step", [(0, 1), (257, 1), (4, -1)])
def test_riqn_loss_rejects_out_of_range_sizes(N, n_step):
    from jorldy_amd import _lib

    lib = _lib.load()
    z = torch.zeros(2, max(N, 1), 2, device="cuda")
    v = torch.zeros(2, device="cuda")
    t = torch.zeros(2, max(N, 1), device="cuda")
    rc = lib.jh_riqn_loss(_lib.ctx(0), 2, 2, N, n_step, _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), _lib.ptr(v), _lib.ptr(v), _lib.ptr(v), _lib.ptr(v), _lib.ptr(t), 0.99, 0.6,
                          _lib.ptr(torch.zeros_like(z)), _lib.ptr(torch.zeros_like(v)), _lib.ptr(torch.zeros(8, device="cuda")), _lib.stream_ptr())
    with pytest.raises(_lib.JhError, match="bad argument"):
        _lib.check(rc)


# ----------------------------------------------------------------------------------------------- the network object
def _mirror64(S, A, E, N, H, noise_type, seed):
    from jorldy_amd.core.network import Network

    torch.manual_seed(seed)
    m = Network("rainbow_iqn", S, A, E, N, noise_type, D_hidden=H).double()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1 and not k.startswith("sig"):
                p.add_(0.05 * torch.randn_like(p))  # biases away from their zero initialisation
            if k.startswith("sig"):
                p.mul_(1.0 + 0.5 * torch.rand_like(p))  # sigmas that differ from weight to weight
    T.round_to_fp32_(m)
    return m, T.as32(m)


def _fwd(mod, x, tau, noise, noise_type):
    return R.riqn_forward(dict(mod.named_parameters()), x, tau, noise, noise_type, next(mod.parameters()).dtype)


@pytest.mark.parametrize("noise_type", ["factorized", "independent"])
@pytest.mark.parametrize("S,A,H,E,N,B", R.NET_SHAPES)
def test_riqnnet_three_forwards_backward_and_adam_match_float64(S, A, H, E, N, B, noise_type):
    """learn_forward, backward (every sig gradient included) and two teacher-forced Adam steps of ops.RainbowIQNNet against float64, at the
    tolerances of test_iqnnet_three_forwards_backward_and_adam_match_float64."""
    from jorldy_amd import ops
    from test_rbnet_gpu import _force, _grads_vs_exact, _native_state

    ref64, ref32 = _mirror64(S, A, E, N, H, noise_type, 0)
    tgt64, tgt32 = _mirror64(S, A, E, N, H, noise_type, 100)
    nat = ops.RainbowIQNNet(S, A, E, N, H, B, "cuda:0", noise_type=noise_type)
    L = R.noise_len(H, A, noise_type)
    assert (nat.maxB, nat.A, nat.K, nat.cnn, nat.noise_len, nat.kind) == (B, A, N, False, L, "rainbow_iqn")
    nat.import_state(ref32.state_dict(), nat.params)
    nat.import_state(tgt32.state_dict(), nat.target)
    sd = nat.export_state()
    assert list(sd.keys()) == list(ref32.state_dict().keys()) == list(R.KEYS)
    for k, v in ref32.state_dict().items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), k
    lr = 1e-3
    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    g = torch.Generator().manual_seed(1)
    for it in range(2):
        _force(nat, truth, lambda step: nat.set_hyper(lr, 0.9, 0.999, 1e-8, step), it)
        x = torch.randn(2 * B, S, generator=g)
        tau = torch.rand(3, B, N, generator=g)
        nz = torch.randn(3, L, generator=g)
        x_dev, tau_dev, nz_dev = x.cuda(), tau.cuda(), nz.cuda()
        out = torch.empty(3, B, N, A, device="cuda")
        nat.learn_forward(x_dev, B, tau_dev, nz_dev, out)
        tn, zn = tau.numpy(), nz.numpy()
        q0, q0_32 = _fwd(ref64, x[:B], tn[0], zn[0], noise_type), _fwd(ref32, x[:B], tn[0], zn[0], noise_type)
        with torch.no_grad():
            q1, q1_32 = _fwd(ref64, x[B:], tn[1], zn[1], noise_type), _fwd(ref32, x[B:], tn[1], zn[1], noise_type)
            q2, q2_32 = _fwd(tgt64, x[B:], tn[2], zn[2], noise_type), _fwd(tgt32, x[B:], tn[2], zn[2], noise_type)
        T.vs_exact(out[0], q0, q0_32, TOL, f"step {it} online(state)")
        T.vs_exact(out[1], q1, q1_32, TOL, f"step {it} online(next_state)")
        T.vs_exact(out[2], q2, q2_32, TOL, f"step {it} target(next_state)")
        if it == 0:  # which = 1 with noise (the agent's target_network view) and without (evaluation); then the learn forward again for backward
            single = nat.forward(x_dev[B:], 1, tau_dev[2], nz_dev[2])
            T.vs_exact(single, q2, q2_32, TOL, "forward(target, next_state, noise)")
            with torch.no_grad():
                e64, e32 = _fwd(ref64, x[:B], tn[0], None, noise_type), _fwd(ref32, x[:B], tn[0], None, noise_type)
            T.vs_exact(nat.forward(x_dev[:B], 0, tau_dev[0], None), e64, e32, TOL, "forward(online, state, no noise)")
            nat.learn_forward(x_dev, B, tau_dev, nz_dev, out)
        gl = torch.randn(B, N, A, generator=g) / (B * N)
        truth.opt64.zero_grad()
        truth.opt32.zero_grad()
        q0.backward(gl.double())
        q0_32.backward(gl)
        nat.backward(gl.cuda().contiguous())
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"step {it} ")
        assert all(float(raw[k].abs().max()) > 0 for k in R.NOISY_KEYS if k.startswith("sig"))
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
    kw = dict(state_size=int(_h(z, "S")), action_size=int(_h(z, "A")), hidden_size=int(_h(z, "H")), num_sample=int(_h(z, "N")), embedding_dim=int(_h(z, "E")),
              noise_type=str(z["hyper/noise_type"]), optim_config=oc, gamma=_h(z, "gamma"), buffer_size=256, batch_size=int(_h(z, "B")), start_train_step=0,
              target_update_period=10000, run_step=100000, n_step=int(_h(z, "n_step")), alpha=_h(z, "alpha"), beta=_h(z, "beta"), learn_period=1,
              uniform_sample_prob=_h(z, "uniform_sample_prob"), device="cuda", use_graph=use_graph)
    kw.update(over)
    return Agent("rainbow_iqn", **kw)


def _initial_weights(z, agent):
    shapes = {k: v.shape for k, v in agent.network.state_dict().items()}
    assert [(k, tuple(int(x) for x in z[f"shape/{k}"])) for k in shapes] == [(k, tuple(v)) for k, v in shapes.items()]
    seed = int(z["recipe_seed"])
    return ({k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed).items()},
            {k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed + 1).items()})


def _thin_cmp(ours, z, prefix, scale_of=None, tol=1e-5, what="", only_stored=False):
    limit, stride = int(z["thin_limit"]), int(z["thin_stride"])
    for k, v in ours.items():
        if only_stored and prefix + k not in z.files:
            continue
        ref = z[prefix + k]
        got = synth.thin(np.asarray(v), limit=limit, stride=stride)
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
    _fill_from_fixture(agent, z, True)
    return agent, w0, wt


def _noise_draws(z, p):
    H, A, nt = int(z["hyper/H"]), int(z["hyper/A"]), str(z["hyper/noise_type"])
    return [{t: tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in pair) for t, pair in R.split_noise(z[p + "noise"][i], H, A, nt).items()} for i in range(3)]


def _reset_tree(agent, z):
    """The priorities the fixture starts from: the same numpy seed then samples the same rows, whatever the last learn() wrote back."""
    agent.memory._tree.load(z["tree0"], float(np.asarray(z["maxp0"]).reshape(-1)[0]), int(z["tree_index0"]), int(z["buf_state"].shape[0]))


def _inject(agent, z, p):
    agent._tau_inject, agent._noise = z[p + "tau"], _noise_draws(z, p)


def _check_learn(agent, z, p, res, tree, result):
    name = p
    assert set(result) == {"loss", "beta", "max_Q", "max_logit", "min_logit", "sampled_p", "mean_p"}
    for k in ("loss", "beta", "max_Q", "max_logit", "min_logit"):
        print(f"{name} result {k}: ours {result[k]!r} reference {float(z[res + k])!r}")
        np.testing.assert_allclose(result[k], z[res + k], rtol=1e-5, err_msg=k)
    np.testing.assert_allclose(result["sampled_p"], z[res + "sampled_p"], rtol=1e-12 if p == "learn/" else 1e-5)
    np.testing.assert_allclose(result["mean_p"], z[res + "mean_p"], rtol=0 if p == "learn/" else 1e-5)
    assert np.array_equal(npy(agent._static["idx"]), z[p + "indices"])  # same sampled rows
    np.testing.assert_allclose(npy(agent._static["w"]), z[p + "weights"].reshape(-1), rtol=1e-6)
    lg = npy(agent._static["logits"])
    for i, k in enumerate(("logit", "logit_next", "logit_target")):  # same sampled rows, same draws, same forwards
        np.testing.assert_allclose(lg[i], z[p + k], rtol=1e-5, atol=1e-5, err_msg=k)
    # the priorities written back: our fp32 loss_b ^ alpha at the sampled leaves, the sums above them
    np.testing.assert_allclose(agent.memory.sum_tree, z[tree], rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("name", FIXTURES)
def test_riqn_agent_learn_matches_reference(name):
    """The assertions and caps of test_iqn_agent_learn_matches_reference with the fixture's tau and noise draws injected, then the second
    recorded learn from the state the first one left, the priorities written back and the tree's sums, sampled_p / mean_p."""
    from test_agents_gpu import _h

    z = load(name)
    agent, w0, wt = _loaded_agent(z)
    assert agent.backend == "native" and agent._net.H == int(_h(z, "H")) and agent._net.kind == "rainbow_iqn"
    _inject(agent, z, "learn/")
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    _check_learn(agent, z, "learn/", "result/", "tree1", result)
    lr = _h(z, "lr")
    _thin_cmp({k: npy(v) for k, v in w0.items()}, z, "sd0_thin/", tol=0.0, what="initial weights", only_stored=True)
    _thin_cmp({k: npy(v) for k, v in wt.items()}, z, "sdt_thin/", tol=0.0, what="target weights", only_stored=True)
    grads = {k: npy(v) for k, v in agent._net.export_state(agent._net.grads).items()}
    _thin_cmp(grads, z, "grad_thin/", scale_of=lambda k: z[f"grad_absmax/{k}"], tol=1e-5, what="d(loss)/d")
    for bucket, nm in ((agent._net.m, "exp_avg"), (agent._net.v, "exp_avg_sq")):
        _thin_cmp({k: npy(v) for k, v in agent._net.export_state(bucket).items()}, z, f"opt1_thin/{nm}/", tol=2e-5, what=nm)
    tot = bad = 0
    worst = 0.0
    limit, stride = int(z["thin_limit"]), int(z["thin_stride"])
    for k, v in agent.network.state_dict().items():
        dd = np.abs(synth.thin(npy(v), limit=limit, stride=stride) - z[f"sd1_thin/{k}"])
        tot += dd.size
        bad += int((dd > 2e-5).sum())
        worst = max(worst, float(dd.max()))
    margins.leq(bad / tot, 0.005, "fraction of weights further than 2e-5 from the reference's")
    margins.leq(worst, 2.1 * lr, "worst weight difference vs the possible travel")
    # ---- the second learn
    _inject(agent, z, "learn2/")
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    _check_learn(agent, z, "learn2/", "learn2/result/", "learn2/tree1", result)


def test_riqn_graph_replay_equals_eager():
    """Five learns with the device's own tau and noise draws: one hipGraph per learn() gives what the eager launches give."""
    z = load("riqn")
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent, _, _ = _loaded_agent(z, use_graph=use_graph, lr=1e-3, run_step=1000)
        np.random.seed(7)
        torch.manual_seed(11)
        out = []
        for it in range(5):
            r = agent.learn()
            agent.learning_rate_decay(10 * (it + 1))
            out.append(r["loss"])
        if use_graph:
            assert agent._graph is not None, "learn() was not captured"
        res.append((out, torch.cat([p.detach().reshape(-1) for p in agent.network.parameters()]).clone(), agent.memory.sum_tree))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=1e-5)


def test_replayed_learns_see_fresh_draws_and_are_bit_equal_when_both_are_injected():
    """Learning rate 0 and the same sampled rows (the tree is put back in front of every learn): consecutive replays differ in their tau and
    noise draws -- and so does the loss; with tau injected alone the noise still moves it; with both injected (the noise written into the
    static buffer) replays give the same bits, and those are the eager call's."""
    z = load("riqn")
    torch.manual_seed(0)
    agent, _, _ = _loaded_agent(z, lr=0.0, lr_decay=False)
    losses = []
    for it in range(4):
        _reset_tree(agent, z)
        np.random.seed(7)
        losses.append(agent.learn()["loss"])
    assert agent._graph is not None
    assert len(set(losses)) == 4
    agent._tau_inject = z["learn/tau"]
    tau_only = []
    for it in range(2):
        _reset_tree(agent, z)
        np.random.seed(7)
        tau_only.append(agent.learn()["loss"])
    assert tau_only[0] != tau_only[1]  # the noise source moved on
    agent._noise = "static"  # the body no longer fills the noise buffer: the graph captured so far does, so it is dropped
    agent.reset_graphs()
    agent._static["noise"].copy_(torch.from_numpy(z["learn/noise"]).cuda())
    fixed, grads = [], []
    for it in range(4):  # captured at the first, replayed after
        _reset_tree(agent, z)
        np.random.seed(7)
        fixed.append(agent.learn()["loss"])
        grads.append(agent._net.grads.clone())
    assert agent._graph is not None
    assert len(set(fixed)) == 1 and fixed[0] not in losses and all(torch.equal(grads[0], g) for g in grads[1:])
    # the eager call's bits
    eager, _, _ = _loaded_agent(z, lr=0.0, lr_decay=False, use_graph=False)
    _inject(eager, z, "learn/")
    np.random.seed(7)
    assert eager.learn()["loss"] == fixed[0] and torch.equal(eager._net.grads, grads[0])


def _truth_actions(agent, states, tau, noise):
    sd = {k: v.cpu() for k, v in agent.network.state_dict().items()}
    with torch.no_grad():
        logits = R.riqn_forward(sd, states, tau, noise, agent.noise_type)
    q = logits.mean(1).numpy()
    top = np.sort(q, -1)
    N = logits.shape[1]
    assert ((top[:, -1] - top[:, -2]) > 2.0 * N * 2.0 ** -24 * np.abs(logits.numpy()).reshape(q.shape[0], -1).max(-1)).all(), "pick states without near-ties"
    return q.argmax(-1)


def test_act_random_until_the_threshold_then_noisy_in_training_and_noise_free_in_evaluation():
    from jorldy_amd.core.agent import Agent
    from test_agents_gpu import _fill_from_fixture

    z = load("riqn")
    S, A, N, H, rows = 4, 3, 8, 64, 5
    torch.manual_seed(0)
    agent = _agent_for(z, start_train_step=50, sample_min=0.25, sample_max=0.25)
    rs = np.random.RandomState(3)
    states = [rs.randn(rows, S).astype(np.float32) for _ in range(6)]
    # ---- below max(batch_size, start_train_step): numpy's stream, nothing else (rainbow_iqn.py:145-149)
    np.random.seed(5)
    ours = [agent.act(s, True)["action"] for s in states]
    np.random.seed(5)
    for a in ours:
        assert a.shape == (rows, 1) and np.array_equal(a, np.random.randint(0, A, size=(rows, 1)))
    _fill_from_fixture(agent, z, True)
    assert agent.memory.size >= 50
    # ---- training: a fresh tau draw from U(0, 1) and a fresh noise draw per call
    seen_noise, seen_tau = [], []
    net = agent._net
    inner_fwd, inner_tau = net.forward, net.draw_tau
    net.forward = lambda x, which=0, tau=None, noise=None, out=None: (seen_noise.append(net.act_noise if noise is None else noise), inner_fwd(x, which, tau, noise, out))[1]
    net.draw_tau = lambda *a, **k: seen_tau.append(inner_tau(*a, **k)) or seen_tau[-1]
    before = np.random.get_state()[1].copy()
    for s in states[:2]:
        a = agent.act(s, True)["action"]
        assert a.shape == (rows, 1) and a.dtype == np.int64
    assert np.array_equal(np.random.get_state()[1], before)  # no epsilon draw
    assert seen_noise[0] is not None and seen_noise[1] is not None and not torch.equal(seen_noise[0], seen_noise[1]) and not torch.equal(seen_tau[0], seen_tau[1])
    assert seen_noise[0].numel() == net.noise_len == R.noise_len(H, A, "factorized")
    big = rs.randn(8, S).astype(np.float32)
    agent.act(big, True)
    t = npy(seen_tau[-1])
    assert t.shape == (8, N) and 0.0 <= t.min() < 0.2 and 0.8 < t.max() <= 1.0
    # ---- ... and the truth's argmax under injected draws
    tau_fixed = rs.rand(rows, N).astype(np.float32)
    agent._tau_inject, agent._noise = tau_fixed, _noise_draws(z, "learn/")
    for s in states:
        assert np.array_equal(agent.act(s, True)["action"].reshape(-1), _truth_actions(agent, s, tau_fixed, z["learn/noise"][0]))
    agent._tau_inject, agent._noise = None, None
    # ---- evaluation: no noise, tau in [sample_min, sample_max]
    greedy = agent.act(big, False)["action"]
    assert seen_noise[-1] is None and np.array_equal(npy(seen_tau[-1]), np.full((8, N), 0.25, np.float32))
    assert np.array_equal(greedy.reshape(-1), _truth_actions(agent, big, np.full((8, N), 0.25, np.float32), None))
    net.forward, net.draw_tau = inner_fwd, inner_tau
    # agent.network / agent.target_network are called as the reference's module is; the target view takes noise too
    logits, tau = agent.network(agent.as_tensor(big), False, 0.25, 0.25)
    assert tuple(logits.shape) == (8, N, A) and tuple(tau.shape) == (8, N, 1) and bool((tau == 0.25).all())
    _, q = agent.logits2Q(logits)
    assert np.array_equal(npy(torch.argmax(q, -1)), greedy.reshape(-1))
    draw = _noise_draws(z, "learn/")[2]
    lt, _ = agent.target_network(agent.as_tensor(big), True, tau=torch.from_numpy(np.full((8, N), 0.25, np.float32)), noise=draw)
    sd_t = {k: v.cpu() for k, v in agent.target_network.state_dict().items()}
    with torch.no_grad():
        want = R.riqn_forward(sd_t, big, np.full((8, N), 0.25, np.float32), z["learn/noise"][2], "factorized")
        want32 = R.riqn_forward(sd_t, big, np.full((8, N), 0.25, np.float32), z["learn/noise"][2], "factorized", torch.float32)
    T.vs_exact(lt, want, want32, TOL, "target_network(x, True) under an injected draw")


def test_checkpoint_roundtrip_keeps_the_reference_order_and_the_noise_stream(tmp_path):
    from test_agents_gpu import _fill_from_fixture

    z = load("riqn")
    a, _, _ = _loaded_agent(z)
    np.random.seed(3)
    a.learn()  # the checkpoint carries Adam moments and a step count
    a.update_target()
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"network", "optimizer"} and list(ckpt["network"].keys()) == list(R.KEYS)
    params = [torch.nn.Parameter(v.clone()) for v in ckpt["network"].values()]  # the reference-ordered parameters
    opt = torch.optim.Adam(params, lr=1e-3)
    opt.load_state_dict(ckpt["optimizer"])
    for p in params:
        assert opt.state[p]["exp_avg"].shape == p.shape and opt.state[p]["exp_avg_sq"].shape == p.shape and float(opt.state[p]["step"]) == 1.0
    ours_m = a._net.export_state(a._net.m)
    for (k, _), p in zip(ckpt["network"].items(), params):
        assert torch.equal(opt.state[p]["exp_avg"], ours_m[k].cpu()), k
    b = _agent_for(z)
    b.load(str(tmp_path))
    _fill_from_fixture(b, z, True)
    b.memory._tree.load(a.memory.sum_tree, float(a.memory.max_priority), int(a.memory.tree_index), a.memory.size)
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, b.network.state_dict()[k]) and torch.equal(v, b.target_network.state_dict()[k]), k
    res = []
    for ag in (a, b):
        np.random.seed(11)
        _inject(ag, z, "learn/")
        res.append(ag.learn())
        ag._tau_inject, ag._noise = None, None
    for k in ("loss", "max_Q", "max_logit", "min_logit", "sampled_p", "mean_p"):
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=1e-6, err_msg=k)
    flat = lambda ag: torch.cat([p.detach().reshape(-1) for p in ag.network.parameters()])
    torch.testing.assert_close(flat(b), flat(a), rtol=1e-5, atol=1e-6)
    # save_full / load_full: buffer, tree, counters, the RNG states and the learner's noise stream survive
    (tmp_path / "full").mkdir()
    a.save_full(str(tmp_path / "full"))
    want = [a.learn() for _ in range(2)]
    d = _agent_for(z)
    d.load_full(str(tmp_path / "full"))
    got = [d.learn() for _ in range(2)]
    for w, g_ in zip(want, got):
        for k in ("loss", "max_Q", "max_logit", "min_logit", "sampled_p"):
            np.testing.assert_allclose(g_[k], w[k], rtol=1e-6, err_msg=f"load_full {k}")


CONFIG = dict(network="rainbow_iqn", optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}, buffer_size=64, batch_size=32, num_sample=64, embedding_dim=64,
              sample_min=0.0, sample_max=1.0, n_step=3, alpha=0.6, beta=0.4, noise_type="factorized", uniform_sample_prob=1e-3, device="cuda")
# config.rainbow_iqn.pong_mlagent's state_size 8 is a multiple of 4: under the eligibility rule it constructs (see the agent's RIQN_ELIGIBLE)
RIQN_SUPPORTED = [("config.rainbow_iqn.cartpole", dict(state_size=4, action_size=2, learn_period=2, target_update_period=1000)),
                  ("config.rainbow_iqn.pong_mlagent", dict(state_size=8, action_size=3, learn_period=4, start_train_step=25000, target_update_period=1000))]
RIQN_REFUSED = [("config.rainbow_iqn.mountaincar", dict(state_size=2, action_size=3)),
                ("config.rainbow_iqn.atari", dict(state_size=(4, 84, 84), action_size=6, head="cnn")),
                ("config.rainbow_iqn.procgen", dict(state_size=(4, 64, 64), action_size=15, head="cnn")),
                ("config.rainbow_iqn.super_mario_bros", dict(state_size=(4, 84, 84), action_size=12, head="cnn"))]


@pytest.mark.parametrize("label,kw", RIQN_SUPPORTED, ids=[c[0] for c in RIQN_SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(CONFIG, **kw)
    agent = Agent("rainbow_iqn", **kw)
    assert agent.backend == "native" and agent.num_support == 64 and agent._net.H == 512 and agent._net.kind == "rainbow_iqn"
    state = np.random.randn(2, kw["state_size"]).astype(np.float32)
    for training in (True, False):  # training below the threshold: random; evaluation: the network + jh_iqn_act
        a = agent.act(state, training)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))
    agent.start_train_step = 0
    agent.memory.first_store = False
    for _ in range(40):  # past the threshold: the noisy network acts
        t = agent.interact_callback({"state": state[:1], "action": np.zeros((1, 1), np.int64), "reward": np.ones((1, 1)), "next_state": state[1:], "done": np.zeros((1, 1), bool)})
        if t:
            agent.memory.store([t])
    assert agent.memory.size >= agent.batch_size
    a = agent.act(state, True)["action"]
    assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))


@pytest.mark.parametrize("label,kw", RIQN_REFUSED, ids=[c[0] for c in RIQN_REFUSED])
def test_reference_configs_outside_the_engine_raise(label, kw):
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.rainbow_iqn import RIQN_ELIGIBLE

    with pytest.raises(ValueError) as e:
        Agent("rainbow_iqn", **dict(CONFIG, **kw))
    assert RIQN_ELIGIBLE in str(e.value)


# ----------------------------------------------------------------------------------------------- learning curve
CURVE_CONFIG = dict(steps=12000, chunk=1000, run_step=15000, hidden_size=128, batch=32, num_sample=32, embedding_dim=64, sample_min=0.0, sample_max=1.0, lr=1e-4,
                    eps=1e-2 / 32, gamma=0.99, start=2000, target=1000, buffer=50000, lr_decay=True, n_step=3, alpha=0.6, beta=0.4, learn_period=2,
                    uniform_sample_prob=1e-3, noise_type="factorized")


class _Windowed:
    """The agent as the single-mode loop drives it (run_mode.py:68-91): every env step goes through interact_callback, and only an assembled
    n-step window reaches process() -- what the reference's side of the curve did (tools/gen_golden_riqn.py)."""

    def __init__(self, agent):
        self.agent = agent

    def act(self, state, training=True):
        return self.agent.act(state, training)

    def process(self, transitions, step):
        windows = [w for w in (self.agent.interact_callback(t) for t in transitions) if w]
        return self.agent.process(windows, step) if windows else {}


def test_riqn_cartpole_learning_curve_tracks_the_reference():
    """config.rainbow_iqn.cartpole at hidden_size 128 and num_sample 32 in the single-mode loop of test_learning_curve_gpu._dqn_curve, three
    seeds, next to the curve of the REAL reference agent on the oracle's bit-identical CartPole (tests/golden/curves_reference_riqn.json).
    The assertions are the IQN curve test's: both start near random play, both learn, and the ends lie within a factor 2 of each other."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from test_learning_curve_gpu import DQN_CHUNK, DQN_RUN_STEP, DQN_STEPS, _dqn_curve

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curves_reference_riqn.json")) as f:
        fx = json.load(f)
    c = CURVE_CONFIG
    assert fx["riqn_cartpole"]["config"] == c
    assert (c["steps"], c["run_step"], c["chunk"]) == (DQN_STEPS, DQN_RUN_STEP, DQN_CHUNK)
    ref = fx["riqn_cartpole"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3 and all(len(r) == DQN_STEPS // DQN_CHUNK for r in ref)

    def gpu_env(seed):
        env = ops.CartPoleVec(1, seed=1000 + seed)
        return env, env.obs().copy()

    def gpu_step(env, action):
        nxt, rew, done = env.step(action)
        return nxt.copy(), rew.reshape(1, 1).astype(np.float64), done.reshape(1, 1).astype(bool), env.obs().copy()

    make = lambda: _Windowed(Agent("rainbow_iqn", state_size=4, action_size=2, hidden_size=c["hidden_size"], network="rainbow_iqn", num_sample=c["num_sample"],
                                   embedding_dim=c["embedding_dim"], sample_min=c["sample_min"], sample_max=c["sample_max"],
                                   optim_config={"name": "adam", "lr": c["lr"], "eps": c["eps"]}, gamma=c["gamma"], buffer_size=c["buffer"], batch_size=c["batch"],
                                   start_train_step=c["start"], target_update_period=c["target"], lr_decay=c["lr_decay"], run_step=c["run_step"], n_step=c["n_step"],
                                   alpha=c["alpha"], beta=c["beta"], learn_period=c["learn_period"], uniform_sample_prob=c["uniform_sample_prob"],
                                   noise_type=c["noise_type"], device="cuda"))
    gpu = [_dqn_curve(make, gpu_env, gpu_step, s) for s in (1, 2, 3)]
    print(json.dumps({"steps": DQN_STEPS, "chunk": DQN_CHUNK, "metric": "mean episode length per 1000 env steps (max 500)", "hip": gpu, "reference": ref}))
    g_start, g_end = np.mean([np.mean(x[:2]) for x in gpu]), np.mean([np.mean(x[-4:]) for x in gpu])
    c_start, c_end = np.mean([np.mean(x[:2]) for x in ref]), np.mean([np.mean(x[-4:]) for x in ref])
    print(f"Rainbow-IQN episode length: HIP {g_start:.1f} -> {g_end:.1f}, reference {c_start:.1f} -> {c_end:.1f}")
    assert g_start < 40 and c_start < 40  # random policy: ~22 steps
    assert g_end > 4 * g_start and c_end > 4 * c_start  # both learn
    assert 0.5 * c_end <= g_end <= 2.0 * c_end
