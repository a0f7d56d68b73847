"""The NoisyNet Q-network kind (jh_rbnet kinds 4 / 5) and the Noisy / Dueling agents on the GPU.

Net parity is against FLOAT64: tests/mirror/noisy.py (network/noisy.py:8-50 on utils.py:55-86 with injectable draws, pinned to the reference's
own forwards by tests/test_noisy_cpu.py) evaluated on the CPU with the same parameters, inputs and draws, torch-CPU float32 beside it --
tests/fp64_truth.py's criterion with TOL = 1e-5, as tests/test_rbnet_gpu.py.  The agent is compared with the reference's own learn()
(fixtures of tools/gen_golden_noisy.py) by the criteria tests/test_mdqn_gpu.py and tests/test_agents_gpu.py use: result scalars at rtol 1e-5,
_cmp_sd for the stepped weights, gradients at 5e-5 max |ref|.  Optimizer moments are functions of the gradient alone after one step from
zero state (exp_avg = 0.1 g, exp_avg_sq = 0.001 g^2), so at the tensor's largest entry they may be off by the gradient's 5e-5 and by twice
that.  Every comparison goes through tests/margins.py."""
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
from tests.util import load, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5
FIXTURES = ["noisy", "noisy_odd", "noisy_cnn"]
# (head, S, A, H, B, noise type): S / batch not multiples of 4 or of a tile, one-channel 36 x 36 frames (1 x 1 feature map), a non-square 2 x 3
# feature map (where the (y, x, c) <-> (c, y, x) permutation of the input-side noise differs from every transpose) with both noise types
CASES = [("mlp", 5, 3, 32, 7, "factorized"), ("mlp", 4, 2, 64, 33, "independent"), ("cnn", (1, 36, 36), 5, 32, 3, "factorized"),
         ("cnn", (4, 44, 52), 6, 32, 8, "factorized"), ("cnn", (4, 44, 52), 6, 32, 8, "independent")]
IDS = [f"{c[0]}-{c[1] if c[0] == 'mlp' else 'x'.join(map(str, c[1]))}-A{c[2]}-H{c[3]}-B{c[4]}-{c[5]}" for c in CASES]


def _net64(S, A, H, head, noise_type, seed):
    from mirror.noisy import Noisy

    torch.manual_seed(seed)
    m = Noisy(S, A, noise_type, D_hidden=H, head=head).double()
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    T.round_to_fp32_(m)
    return m, T.as32(m)


def _mk(head, S, A, H, B, noise_type, seed=0):
    from jorldy_amd import ops

    ref64, ref32 = _net64(S, A, H, head, noise_type, seed)
    tgt64, tgt32 = _net64(S, A, H, head, noise_type, seed + 100)
    nat = ops.RainbowNet(S, A, 1, H, head, B, "cuda:0", kind="noisy", noise_type=noise_type)
    nat.import_state(ref32.state_dict(), nat.params)
    nat.import_state(tgt32.state_dict(), nat.target)
    assert list(nat.export_state().keys()) == list(ref32.state_dict().keys())
    F = ref32.mu_w1.shape[0]
    assert nat.noise_len == (F * H + H + H * A + A if noise_type == "independent" else F + 2 * H + A)
    return (ref64, ref32), (tgt64, tgt32), nat, F


def _np_stream():
    """Where numpy's global generator stands (key words and position)."""
    st = np.random.get_state()
    return st[1].tobytes(), int(st[2])


def _dicts(noise, F, H, A, noise_type):
    from mirror.noisy import noise_dicts

    return noise_dicts(noise, F, H, A, noise_type, torch.float64), noise_dicts(noise, F, H, A, noise_type, torch.float32)


# ----------------------------------------------------------------------------------------------- the network against float64
@pytest.mark.parametrize("head,S,A,H,B,nt", CASES, ids=IDS)
def test_noisy_net_forwards_backward_and_sigma_mean_match_float64(head, S, A, H, B, nt):
    from test_rbnet_gpu import _grads_vs_exact, _inputs

    (ref64, ref32), (tgt64, tgt32), nat, F = _mk(head, S, A, H, B, nt)
    g = torch.Generator().manual_seed(1)
    x_dev, x64 = _inputs(head, S, 2 * B, g)
    x32 = x64.float()
    noise = torch.randn(2, nat.noise_len, generator=g)
    noise_dev = noise.cuda()  # stays alive until after backward(): the sigma gradients re-read the draws
    nd64, nd32 = _dicts(noise, F, H, A, nt)
    # network(x, is_train): with a draw, and without one = mu only
    xs = x_dev[:B].contiguous()
    with torch.no_grad():
        T.vs_exact(nat.forward(xs, which=0, noise=noise_dev[1])[:, :, 0], ref64(x64[:B], True, nd64[1]), ref32(x32[:B], True, nd32[1]), TOL, "forward with a draw")
        T.vs_exact(nat.forward(xs, which=1, noise=None)[:, :, 0], tgt64(x64[:B], False), tgt32(x32[:B], False), TOL, "forward without a draw (mu only)")
        zero = torch.zeros(nat.noise_len, device="cuda")
        assert torch.equal(nat.forward(xs, which=1, noise=None), nat.forward(xs, which=1, noise=zero)), "no draw = a draw of zeros = mu"
    # the two forwards of learn()
    out = torch.full((2, B, A, 1), float("nan"), device="cuda")
    nat.learn_forward_n(x_dev, B, noise_dev, out)
    q0, q0_32 = ref64(x64[:B], True, nd64[0]), ref32(x32[:B], True, nd32[0])
    with torch.no_grad():
        q1, q1_32 = tgt64(x64[B:], True, nd64[1]), tgt32(x32[B:], True, nd32[1])
        other = ref64(x64[:B], True, nd64[1])
    assert float((other - q0.detach()).abs().max()) > 1e-2 * float(q0.detach().abs().max()), "the draws differ enough to tell the forwards apart"
    T.vs_exact(out[0, :, :, 0], q0, q0_32, TOL, "online(state; draw 0)")
    T.vs_exact(out[1, :, :, 0], q1, q1_32, TOL, "target(next_state; draw 1)")
    gl = torch.randn(B, A, generator=g) / B
    q0.backward(gl.double())
    q0_32.backward(gl)
    gl_dev = gl.cuda().contiguous()
    nat.backward(gl_dev)
    _grads_vs_exact(nat, ref64, ref32)
    for k in ("sig_w1", "sig_b1", "sig_w2", "sig_b2"):
        assert float(dict(ref64.named_parameters())[k].grad.abs().max()) > 0, k
    # the deferred backward completes in flush_grads with the same bytes
    plain = nat.grads.clone()
    nat.grads.zero_()
    nat.learn_forward_n(x_dev, B, noise_dev, out)
    nat.backward(gl_dev, defer=True)
    nat.flush_grads()
    assert torch.equal(nat.grads, plain)
    # Noisy.get_sig_w_mean
    s = nat.sig_abs_mean()
    s_again = nat.sig_abs_mean()
    torch.cuda.synchronize()
    assert torch.equal(s, s_again)
    with torch.no_grad():
        for i, (e64, e32) in enumerate(zip(ref64.get_sig_w_mean(), ref32.get_sig_w_mean())):
            T.vs_exact(s[i : i + 1], e64.reshape(1), e32.reshape(1), TOL, f"mean |sig_w{i + 1}|")


@pytest.mark.parametrize("nt", ["factorized", "independent"])
def test_learn_forward_n_runs_each_trunk_over_its_own_half_only(nt):
    """The online forward reads rows [0, B) and the target forward rows [B, 2B): NaN in the other half leaves a forward's bits alone."""
    head, S, A, H, B = "mlp", 5, 3, 32, 7
    _, _, nat, _ = _mk(head, S, A, H, B, nt)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2 * B, S, generator=g).cuda()
    noise = torch.randn(2, nat.noise_len, generator=g).cuda()
    clean = nat.learn_forward_n(x, B, noise, torch.empty(2, B, A, 1, device="cuda")).clone()
    assert bool(torch.isfinite(clean).all())
    hi, lo = x.clone(), x.clone()
    hi[B:] = float("nan")
    lo[:B] = float("nan")
    out_hi = nat.learn_forward_n(hi, B, noise, torch.empty(2, B, A, 1, device="cuda")).clone()
    out_lo = nat.learn_forward_n(lo, B, noise, torch.empty(2, B, A, 1, device="cuda")).clone()
    assert torch.equal(out_hi[0], clean[0]) and not torch.equal(out_hi[1], clean[1])
    assert torch.equal(out_lo[1], clean[1]) and not torch.equal(out_lo[0], clean[0])
    swapped = nat.learn_forward_n(x, B, noise.flip(0).contiguous(), torch.empty(2, B, A, 1, device="cuda"))
    assert not torch.equal(swapped[0], clean[0]) and not torch.equal(swapped[1], clean[1]), "each forward uses its own draw"


@pytest.mark.parametrize("head,S,A,H,B,nt", [CASES[0], CASES[4]], ids=[IDS[0], IDS[4]])
def test_noisy_net_adam_and_centered_rmsprop_steps_match_float64(head, S, A, H, B, nt):
    """Three teacher-forced Adam steps through the deferred backward, then one step of centered RMSprop with a clip that bites."""
    from test_rbnet_gpu import _force, _grads_vs_exact, _inputs, _native_state

    (ref64, ref32), _, nat, F = _mk(head, S, A, H, B, nt, seed=5)
    g = torch.Generator().manual_seed(2)
    lr = 1e-3

    def one_step(truth, set_hyper, it, optimizer, clip, tag):
        _force(nat, truth, set_hyper, it)
        x_dev, x64 = _inputs(head, S, 2 * B, g)
        noise = torch.randn(2, nat.noise_len, generator=g)
        noise_dev = noise.cuda()
        nat.learn_forward_n(x_dev, B, noise_dev, torch.empty(2, B, A, 1, device="cuda"))
        gl = torch.randn(B, A, generator=g)
        nd = _dicts(noise, F, H, A, nt)
        for m, opt, dt, d in ((ref64, truth.opt64, torch.float64, nd[0]), (ref32, truth.opt32, torch.float32, nd[1])):
            opt.zero_grad()
            m(x64[:B].to(dt), True, d[0]).backward(gl.to(dt))
        nat.backward(gl.cuda().contiguous(), defer=True)
        nat.flush_grads()
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"{tag} {it} ")
        nat.optim_step(optimizer, clip)
        truth.step(clip, raw, *_native_state(nat), tag=f"{tag} {it}")

    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    for it in range(3):
        one_step(truth, lambda step: nat.set_hyper(lr, 0.9, 0.999, 1e-8, step), it, "adam", None, "adam step")
    lr2 = 2.5e-4
    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.RMSprop(ps, lr=lr2, alpha=0.95, eps=1.5e-7, centered=True), lr2, ("grad_avg", "square_avg"))
    one_step(truth, lambda step: nat.set_hyper(lr2, 0.95, 0.0, 1.5e-7, step, centered=True), 0, "rmsprop", 0.5, "rmsprop step")


def test_sigma_mean_at_atari_shape_and_under_graph_replay():
    """512 x 3136 sigmas: every workgroup of the reduction has work; eager twice and a graph replay return the same bits."""
    from jorldy_amd import ops

    nat = ops.RainbowNet((4, 84, 84), 6, 1, 512, "cnn", 1, "cuda:0", kind="noisy")
    torch.manual_seed(4)
    sd = nat.export_state()
    for k in ("sig_w1", "sig_w2"):
        sd[k] = (0.02 * torch.randn(sd[k].shape)).float()
    nat.import_state(sd)
    a, b = nat.sig_abs_mean().clone(), nat.sig_abs_mean().clone()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    out = torch.zeros(2, device="cuda")
    with ops.graph_capture(graph):
        nat.sig_abs_mean(out)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)
    assert torch.equal(a, b)
    for i, k in enumerate(("sig_w1", "sig_w2")):
        T.vs_exact(a[i : i + 1], sd[k].double().abs().mean().reshape(1), sd[k].abs().mean().reshape(1), TOL, f"mean |{k}| at atari shape")


# ----------------------------------------------------------------------------------------------- refusals
def test_other_learn_entries_refuse_the_noisy_network():
    from jorldy_amd import _lib as L

    B, A = 4, 3
    for nt, kind in (("factorized", 4), ("independent", 5)):
        _, _, nat, _ = _mk("mlp", 4, A, 32, B, nt)
        x = torch.zeros(2 * B, 4, device="cuda")
        noise = torch.zeros(3, nat.noise_len, device="cuda")
        out = torch.empty(3, B, A, 1, device="cuda")
        v = torch.zeros(B, 1, device="cuda")
        calls = {"learn_forward": lambda: nat.learn_forward(x, B, noise, out), "learn_forward_m": lambda: nat.learn_forward_m(x, B, noise, out),
                 "learn_forward_p": lambda: nat.learn_forward_p(x, B, noise, out),
                 "c51_step": lambda: nat.c51_step(None, None, v, v, v, None, -1.0, 1.0, 0.99, 0.6, 1, out)}
        for name, call in calls.items():
            with pytest.raises(L.JhError, match=f"kind {kind}") as e:
                call()
            assert name in str(e.value), (name, str(e.value))
    from jorldy_amd import ops

    plain = ops.RainbowNet(4, A, 1, 32, "mlp", B, "cuda:0", kind="q")
    with pytest.raises(L.JhError):
        plain.learn_forward_n(torch.zeros(2 * B, 4, device="cuda"), B, torch.zeros(2, 8, device="cuda"), torch.empty(2, B, A, 1, device="cuda"))
    with pytest.raises(L.JhError):
        plain.sig_abs_mean()


def test_unsupported_configurations_raise_at_construction():
    from jorldy_amd.core.agent import Agent

    base = dict(state_size=4, action_size=2, hidden_size=64, optim_config={"name": "adam", "lr": 1e-4}, device="cuda")
    for name, kw in (("dqn", dict(network="noisy")), ("m_dqn", dict(network="noisy")), ("per", dict(network="noisy")), ("noisy", dict(network="dueling")),
                     ("dueling", dict(network="discrete_q_network"))):
        with pytest.raises(ValueError):
            Agent(name, **dict(base, **kw))
    for kw in (dict(noise_type="gaussian_process"), dict(hidden_size=30), dict(optim_config={"name": "sgd", "lr": 1e-3}), dict(head="multi")):
        with pytest.raises(ValueError, match="libjorldy_hip") as e:
            Agent("noisy", **dict(base, **kw))
        assert "network 'noisy'" in str(e.value) and "got network='noisy'" in str(e.value)


# ----------------------------------------------------------------------------------------------- the agent against the reference
def _agent_for(z, lr=None, **over):
    from jorldy_amd.core.agent import Agent
    from test_agents_gpu import _h

    S = z["hyper/S"]
    cnn = S.ndim > 0
    kw = dict(state_size=tuple(int(v) for v in S) if cnn else int(S), action_size=int(_h(z, "A")), hidden_size=int(_h(z, "H")), head=str(z["hyper/head"]),
              noise_type=str(z["hyper/noise_type"]), optim_config={"name": "adam", "lr": _h(z, "lr") if lr is None else lr}, gamma=_h(z, "gamma"),
              buffer_size=64 if cnn else 256, batch_size=int(_h(z, "B")), start_train_step=0, target_update_period=10000, run_step=100000, device="cuda")
    kw.update(over)
    return Agent("noisy", **kw)


def _initial_weights(z, agent):
    from oracle import synth
    from test_agents_gpu import _sd

    if "recipe_seed" not in z.files:
        return _sd(z, "sd0/"), _sd(z, "sdt/")
    shapes = {k: v.shape for k, v in agent.network.state_dict().items()}
    seed = int(z["recipe_seed"])
    return ({k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed).items()},
            {k: torch.from_numpy(v) for k, v in synth.recipe_state_dict(shapes, seed + 1).items()})


def _loaded_agent(z, **over):
    from test_agents_gpu import _fill_from_fixture

    agent = _agent_for(z, **over)
    w0, wt = _initial_weights(z, agent)
    agent.network.load_state_dict(w0)
    agent.target_network.load_state_dict(wt)
    _fill_from_fixture(agent, z, False)
    return agent, w0, wt


@pytest.mark.parametrize("name", FIXTURES)
def test_noisy_agent_learn_matches_reference(name):
    """The reference draws its NoisyNet noise with torch's CPU generator inside forward (utils.py:58-60, 75-76); the same draws are regenerated
    (same seed, same order) and injected, so that the whole update is comparable."""
    from oracle import synth
    from test_agents_gpu import _cmp_sd, _h, _sd
    from test_baseline_width_gpu import _thin_cmp
    from test_noisy_cpu import regenerate_draws

    z = load(name)
    agent, w0, wt = _loaded_agent(z)
    assert agent.backend == "native" and agent._net.kind == "noisy"
    if name == "noisy_cnn":
        assert agent.memory._store.column("state").dtype == torch.uint8  # frames stay uint8 in HBM
    A, H, B = int(_h(z, "A")), int(_h(z, "H")), int(_h(z, "B"))
    agent._noise = regenerate_draws(z, int(w0["mu_w1"].shape[0]), H, A)
    np.random.seed(int(_h(z, "np_seed")))
    result = agent.learn()
    assert set(result) == {"loss", "max_Q", "sig_w1", "sig_w2"}
    for k in sorted(result):
        print(f"{name} result {k}: ours {result[k]!r} reference {float(z[f'result/{k}'])!r}")
    for k in sorted(result):
        np.testing.assert_allclose(result[k], z[f"result/{k}"], rtol=1e-5, err_msg=k)
    lg = npy(agent._static["logits"]).reshape(3, B, A)
    for i, k in enumerate(("q_all", "next_q")):  # same sampled rows, same draws, both forwards
        np.testing.assert_allclose(lg[i], z[f"learn/{k}"], rtol=1e-5, atol=1e-5, err_msg=k)
    lr = _h(z, "lr")
    grads = {k: npy(v) for k, v in agent._net.export_state(agent._net.grads).items()}
    moments = {nm: {k: npy(v) for k, v in agent._net.export_state(bucket).items()} for bucket, nm in ((agent._net.m, "exp_avg"), (agent._net.v, "exp_avg_sq"))}
    m_tol = {"exp_avg": 5e-5, "exp_avg_sq": 1e-4}  # (module docstring)
    if "recipe_seed" not in z.files:
        for k, v in grads.items():
            ref = z[f"grad/{k}"]
            margins.leq(float(np.abs(v - ref).max()), 5e-5 * (float(np.abs(ref).max()) + 1e-12) + 1e-9, f"{name} grad {k}")
        for nm, d in moments.items():
            for k, v in d.items():
                ref = z[f"opt1/{nm}/{k}"]
                margins.leq(float(np.abs(v - ref).max()), m_tol[nm] * float(np.abs(ref).max()) + 1e-12, f"{name} {nm} {k}")
        _cmp_sd(agent.network, _sd(z, "sd1/"), lr, 1)
        return
    _thin_cmp({k: npy(v) for k, v in w0.items()}, z, "sd0_thin/", tol=0.0, what="initial weights")
    _thin_cmp({k: npy(v) for k, v in wt.items()}, z, "sdt_thin/", tol=0.0, what="target weights")
    _thin_cmp(grads, z, "grad_thin/", scale_of=lambda k: z[f"grad_absmax/{k}"], tol=5e-5, what="d(loss)/d")
    for nm, d in moments.items():
        _thin_cmp(d, z, f"opt1_thin/{nm}/", tol=m_tol[nm], what=nm)
    tot = bad = 0
    worst = 0.0
    for k, v in agent.network.state_dict().items():  # _cmp_sd on the thinned tensors
        dd = np.abs(synth.thin(npy(v)) - z[f"sd1_thin/{k}"])
        tot += dd.size
        bad += int((dd > 2e-5).sum())
        worst = max(worst, float(dd.max()))
    margins.leq(bad / tot, 0.005, "fraction of weights further than 2e-5 from the reference's")
    margins.leq(worst, 2.1 * lr, "worst weight difference vs the possible travel")


def _static_noise(agent, seed):
    agent._noise = "static"
    agent._static = agent._alloc_static()
    agent.reset_graphs()
    agent._static["noise"].copy_(torch.randn(agent._static["noise"].shape, generator=torch.Generator().manual_seed(seed)))


def test_noisy_graph_replay_equals_eager():
    """The assertions of test_mdqn_graph_replay_equals_eager, with the same draws in the static noise buffer of both runs."""
    z = load("noisy")
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent, _, _ = _loaded_agent(z, use_graph=use_graph, lr=1e-3, run_step=1000)
        _static_noise(agent, 5)
        np.random.seed(7)
        out = []
        for it in range(5):
            r = agent.learn()
            agent.learning_rate_decay(10 * (it + 1))
            out.append([r["loss"], r["sig_w1"], r["sig_w2"]])
        if use_graph:
            assert agent._graph is not None, "learn() was not captured"
        else:
            assert agent._graph is None
        res.append((out, torch.cat([p.detach().reshape(-1) for p in agent.network.parameters()]).clone()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)


def test_device_noise_is_fresh_per_replay_and_resumes(tmp_path):
    """With the device noise source a replayed graph draws new noise every time; save_full / load_full carry the stream."""
    z = load("noisy")

    def mk():
        torch.manual_seed(0)
        np.random.seed(0)
        return _loaded_agent(z, lr=1e-3, run_step=1000)[0]

    a = mk()
    torch.manual_seed(3)
    seen = []
    for _ in range(4):
        a.learn()
        seen.append((a._static["noise"].clone(), a._static["logits"][:2].clone()))
    assert a._graph is not None
    assert not torch.equal(seen[2][0], seen[3][0]) and not torch.equal(seen[2][1], seen[3][1]), "two consecutive replays: other noise, other logits"
    assert float(seen[3][0].std()) > 0.5
    os.makedirs(tmp_path / "ck")
    a.save_full(str(tmp_path / "ck"))
    want = [a.learn() for _ in range(3)]
    want_noise = a._static["noise"].clone()
    b = mk()
    torch.manual_seed(12345)  # whatever the process' torch generator holds: the restored stream must not depend on it
    b.load_full(str(tmp_path / "ck"))
    got = [b.learn() for _ in range(3)]
    assert torch.equal(b._static["noise"], want_noise), "the resumed run drew the noise of the uninterrupted one"
    for w, r in zip(want, got):  # (a replays its graph, b starts eagerly: the comparison of test_noisy_graph_replay_equals_eager)
        np.testing.assert_allclose([r[k] for k in sorted(r)], [w[k] for k in sorted(w)], rtol=1e-5)
    torch.testing.assert_close(a._net.params, b._net.params, rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------------------------------------- acting
def test_act_warm_up_draws_randint_alone_then_follows_the_network():
    z = load("noisy")
    agent, _, _ = _loaded_agent(z, start_train_step=10 ** 6)  # warm-up: memory.size < start_train_step
    A = agent.action_size
    x = np.random.RandomState(1).randn(5, 4).astype(np.float32)
    np.random.seed(9)
    a = agent.act(x, training=True)["action"]
    tail = np.random.random(3)
    np.random.seed(9)
    want = np.random.randint(0, A, size=(5, 1))
    assert np.array_equal(a, want) and a.shape == (5, 1)
    assert np.array_equal(np.random.random(3), tail), "the numpy stream advanced by that one call (no epsilon draw)"
    # evaluation never takes the warm-up branch
    xd = torch.from_numpy(x).cuda()
    greedy = npy(agent._net.forward(xd, which=0, noise=None))[:, :, 0].argmax(-1).reshape(-1, 1)
    state = _np_stream()
    for _ in range(2):
        assert np.array_equal(agent.act(x, training=False)["action"], greedy)
    assert _np_stream() == state, "no host draw at all"
    # after warm-up
    agent.start_train_step = 0
    assert agent.memory.size >= agent.batch_size
    for _ in range(2):
        assert np.array_equal(agent.act(x, training=False)["action"], greedy)
    torch.manual_seed(1)
    q = [agent.network(xd, True).clone() for _ in range(2)]
    assert q[0].shape == (5, A) and not torch.equal(q[0], q[1]), "training mode: a fresh draw per call"
    acts = [agent.act(x, training=True)["action"] for _ in range(3)]
    assert all(t.shape == (5, 1) and t.dtype == np.int64 and np.all((t >= 0) & (t < A)) for t in acts)
    assert torch.equal(agent.network(xd, False), agent.network(xd, False)) and torch.equal(agent.network(xd, False).argmax(-1, keepdim=True).cpu(), torch.from_numpy(greedy))


SUPPORTED = [
    ("cartpole", dict(state_size=4, action_size=2)),
    ("mountaincar", dict(state_size=2, action_size=3)),
    ("pong_mlagent", dict(state_size=8, action_size=3)),
    ("atari", dict(state_size=(4, 84, 84), action_size=6, head="cnn")),
    ("procgen", dict(state_size=(3, 64, 64), action_size=15, head="cnn")),
]


@pytest.mark.parametrize("agent_name", ["noisy", "dueling"])
@pytest.mark.parametrize("label,kw", SUPPORTED, ids=[c[0] for c in SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw, agent_name):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    kw = dict(dict(hidden_size=64, optim_config={"name": "adam", "lr": 1e-4}, buffer_size=64, batch_size=8, device="cuda"), **kw)
    if agent_name == "dueling" and label == "atari":
        kw["network"] = "dueling"  # config.dueling.* give the key; the other shapes take the default
    agent = Agent(agent_name, **kw)
    assert agent.backend == "native" and agent._net.kind == agent_name
    S = kw["state_size"]
    state = np.random.randint(0, 256, size=(2,) + tuple(S), dtype=np.uint8) if isinstance(S, tuple) else np.random.randn(2, S).astype(np.float32)
    for training in (True, False):
        a = agent.act(state, training)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))
    if agent_name == "noisy":
        agent.start_train_step = 0
        agent.batch_size = 0  # past the warm-up branch with an empty replay: the noisy network acts
        a = agent.act(state, True)["action"]
        assert a.shape == (2, 1) and np.all((a >= 0) & (a < kw["action_size"]))


def test_initial_weights_are_the_reference_agents_third_construction():
    """noisy.py:38-65: DQN.__init__ builds two networks, Noisy.__init__ two more and keeps the first of those."""
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.network import Network

    for nt in ("factorized", "independent"):
        torch.manual_seed(21)
        agent = Agent("noisy", state_size=4, action_size=3, hidden_size=32, noise_type=nt, buffer_size=64, batch_size=8, device="cuda")
        torch.manual_seed(21)
        for _ in range(2):
            Network("noisy", 4, 3, D_hidden=32, head="mlp")
        third = Network("noisy", 4, 3, nt, D_hidden=32, head="mlp")
        sd = agent.network.state_dict()
        assert list(sd) == list(third.state_dict())
        for k, v in third.state_dict().items():
            assert torch.equal(sd[k].cpu(), v) and torch.equal(agent.target_network.state_dict()[k].cpu(), v), k


# ----------------------------------------------------------------------------------------------- actors, checkpoints, Dueling
def test_batched_actors_on_a_noisy_agent():
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import BatchedValueActors

    torch.manual_seed(1)
    np.random.seed(1)
    A, N, S = 5, 9, 6
    agent = Agent("noisy", state_size=S, action_size=A, hidden_size=32, batch_size=8, buffer_size=64, start_train_step=0, device="cuda")
    with torch.no_grad():
        agent._net.params.add_(0.05 * torch.randn_like(agent._net.params))
    actors = BatchedValueActors(agent, N)
    assert actors.noisy and not actors.eps.any()
    obs = np.random.RandomState(2).randn(N, S).astype(np.float32)
    out = actors.act(obs, training=False)
    for i in range(N):
        ref = agent.act(obs[i : i + 1], training=False)
        assert int(ref["action"][0, 0]) == int(out["action"][i, 0]), i
    again = actors.act(obs, training=False)
    assert np.array_equal(again["q"], out["q"])
    qs, draws = [], []
    state = _np_stream()
    for _ in range(2):
        qs.append(actors.act(obs, training=True)["q"].copy())
        actors.stream.synchronize()
        draws.append(actors._noise.clone())
    assert not torch.equal(draws[0], draws[1]) and not np.array_equal(qs[0], qs[1]), "a fresh draw per tick"
    assert _np_stream() == state, "epsilon 0: no host draw"
    np.random.seed(5)
    a = actors.act(obs, training=True, random_actions=True)["action"]
    np.random.seed(5)
    np.random.random(N)
    assert np.array_equal(a[:, 0], np.random.randint(0, A, size=N)), "the warm-up path is what it was"


def test_checkpoint_roundtrip_in_the_references_format(tmp_path):
    z = load("noisy")
    a, _, _ = _loaded_agent(z)
    np.random.seed(3)
    a.learn()
    a.learning_rate_decay(500)
    a.update_target()
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"network", "optimizer"}
    assert list(ckpt["network"])[:8] == ["mu_w1", "sig_w1", "mu_b1", "sig_b1", "mu_w2", "sig_w2", "mu_b2", "sig_b2"] and list(ckpt["network"])[8:] == ["head.l.weight", "head.l.bias"]
    assert tuple(ckpt["network"]["mu_w1"].shape) == (32, 32) and tuple(ckpt["network"]["mu_w2"].shape) == (32, 3)
    assert set(ckpt["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and len(ckpt["optimizer"]["state"]) == 10
    b, _, _ = _loaded_agent(z)
    b.load(str(tmp_path))
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, b.network.state_dict()[k]) and torch.equal(v, b.target_network.state_dict()[k]), k
    assert torch.equal(a._net.m, b._net.m) and torch.equal(a._net.v, b._net.v)
    assert b._adam_steps == a._adam_steps == 1 and b._lr_now == a._lr_now != a._lr0
    for ag in (a, b):
        _static_noise(ag, 8)
    res = []
    for ag in (a, b):
        np.random.seed(11)
        res.append(ag.learn())
    for k in res[0]:
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=1e-6, err_msg=k)
    c = _agent_for(z)
    c.sync_in(a.sync_out()["weights"])
    for k, v in a.network.state_dict().items():
        assert torch.equal(v, c.network.state_dict()[k]), k


def test_dueling_learn_is_bit_identical_to_dqn_on_the_dueling_network():
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.dqn import DQN
    from jorldy_amd.core.agent.dueling import Dueling

    z = load("dqn")
    from test_agents_gpu import _fill_from_fixture, _h

    res = []
    for name, kw in (("dueling", {}), ("dueling", dict(network="dueling")), ("dqn", dict(network="dueling"))):
        torch.manual_seed(2)
        np.random.seed(2)
        agent = Agent(name, state_size=int(_h(z, "S")), action_size=int(_h(z, "A")), hidden_size=int(_h(z, "H")), optim_config={"name": "adam", "lr": 1e-3},
                      buffer_size=256, batch_size=int(_h(z, "B")), start_train_step=0, device="cuda", **kw)
        assert agent._net.kind == "dueling" and type(agent) is (Dueling if name == "dueling" else DQN)
        _fill_from_fixture(agent, z, False)
        np.random.seed(4)
        out = [agent.learn() for _ in range(3)]
        res.append((out, agent._net.params.clone(), agent._net.m.clone(), agent._net.v.clone()))
    for r in res[:2]:
        assert r[0] == res[2][0] and set(r[0][0]) == {"loss", "epsilon", "max_Q"}
        for a, b in zip(r[1:], res[2][1:]):
            assert torch.equal(a, b)
