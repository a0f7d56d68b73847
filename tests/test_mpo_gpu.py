"""Discrete MPO on the GPU: the loss kernel against the float64 truth of tests/mpo_truth.py over every block shape the launch takes, the
multipliers' device-side Adam step as arithmetic, determinism and argument checks; the actor's three forwards against three separate forwards;
the agent against the reference's fixtures (tools/gen_golden_mpo.py), graph replay against eager bit for bit, checkpoints, the reference's
configurations, act()'s probabilities, and one CartPole learning curve against the unmodified reference's."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import mpo_truth as D
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_vmpo_gpu.py's
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the loss kernel
def _run_kernel(c, retrace=True, has_state=(True, True, False)):
    """-> (grads {"la", "q"}, stats [11], block after (ops.vmpo_block_read), raw block before, raw block after)"""
    from jorldy_amd import ops

    blk = ops.vmpo_block(*[float(x) for x in c["mult"]], *[float(x) for x in c["floors"]], c["eps"][0], c["eps"][1], 0.1, m=c["m"], v=c["v"], has_state=has_state)
    blk[:3] = f32(c["mult"])  # exactly the case's values
    before = npy(blk).copy()
    hyper = ops.vmpo_hyper(D.LR, D.BETAS[0], D.BETAS[1], D.ADAM_EPS, D.STEP0)
    g_la, g_q, stats = ops.mpo_loss_discrete(*[f32(v) for v in D.case_args(c)], c["T"], blk, hyper, c["gamma"], retrace=retrace)
    torch.cuda.synchronize()
    return {"la": npy(g_la), "q": npy(g_q)}, npy(stats).copy(), ops.vmpo_block_read(blk), before, npy(blk).copy()


def _scalar(ours, exact, ref32, what):
    """tests/test_vmpo_gpu.py's rule: |ours - exact| / |exact| <= max(TOL, 2 x the float32 reference's own error); a float32 reference that is
    inf or NaN (the `hot` case) leaves TOL."""
    scale = abs(exact) + 1e-30
    e_ref = abs(ref32 - exact) / scale if np.isfinite(ref32) else 0.0
    err = abs(float(ours) - exact) / scale
    print(f"{what}: ours {float(ours)!r} fp64 {exact!r} error {err:.2e} (reference fp32: {e_ref:.2e})")
    margins.leq(err, max(TOL, 2.0 * e_ref), f"{what} |ours - fp64| / |fp64| (reference fp32: {e_ref:.2e})")


def _check_case(c, retrace, what, against_fp32=True):
    t64 = D.case_truth(c, retrace)
    t32 = D.case_truth(c, retrace, torch.float32) if against_fp32 else None
    grads, stats, blk, raw0, raw1 = _run_kernel(c, retrace)
    R, A = c["la"].shape
    for k, g in grads.items():
        assert np.isfinite(g).all(), f"{what}: d {k}"
        T.grad_vs_exact(g, t64["grads"][k], t32["grads"][k] if t32 else None, TOL, f"{what} d(loss)/d {k}")
    other = np.ones((R, A), bool)
    other[np.arange(R), c["action"].astype(np.int64)] = False
    assert not grads["q"][other].any(), "entries of the actions not taken are written as zeros"
    for j, key in enumerate(("actor", "critic", "eta_loss", "alpha_loss")):
        assert np.isfinite(stats[j]), f"{what}: {key}"
        _scalar(stats[j], t64[key], t32[key] if t32 else float("nan"), f"{what} {key}")
    for j in range(2):
        n = D.NAMES[j]
        g = blk[n]["grad"]
        e_ref = abs(t32["mult_grads"][j] - t64["mult_grads"][j]) / t64["mult_scale"][j] if (t32 and np.isfinite(t32["mult_grads"][j])) else 0.0
        margins.leq(abs(g - t64["mult_grads"][j]) / t64["mult_scale"][j], max(TOL, 2.0 * e_ref), f"{what} d(loss)/d {n} against the magnitude of its terms")
        x0 = float(c["mult"][j])
        w, m, v = D.multiplier_step(x0, g, c["m"][j], c["v"][j], D.STEP0, D.LR, c["floors"][j], D.BETAS, D.ADAM_EPS)
        margins.leq(abs(blk[n]["value"] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * D.LR, f"{what} {n} after float64 Adam on OUR gradient")
        margins.leq(abs(blk[n]["m"] - m), 1e-5 * abs(m), f"{what} {n} exp_avg")
        margins.leq(abs(blk[n]["v"] - v), 1e-5 * abs(v), f"{what} {n} exp_avg_sq")
        assert blk[n]["has_state"] and stats[4 + j] == np.float32(blk[n]["value"])
    for off in (2, 5, 8, 17, 20):  # value, exp_avg, exp_avg_sq, has-state flag, last gradient of alpha_sigma
        assert raw0[off].tobytes() == raw1[off].tobytes(), f"{what}: a discrete policy leaves alpha_sigma's block entry {off} untouched"
    assert not blk["alpha_sigma"]["has_state"] and stats[6] == c["mult"][2] and raw0[9:15].tobytes() == raw1[9:15].tobytes()
    # extrema over ALL [R, A] entries.  q is an input: exact.  At is a float64 value rounded once to float32; the truth's V may differ from the
    # kernel's in the last bits of a double (summation order), so the two roundings differ by at most one float32 ulp
    assert (stats[7], stats[8]) == (np.float32(t64["extrema"][0]), np.float32(t64["extrema"][1])) == (c["q"].min(), c["q"].max())
    for j in (2, 3):
        margins.leq(abs(float(stats[7 + j]) - t64["extrema"][j]), 2.0 ** -23 * abs(t64["extrema"][j]), f"{what} {'min' if j == 2 else 'max'} At within one float32 ulp")
    return stats, blk


@pytest.mark.parametrize("B,T_,A", D.KERNEL_CASES, ids=[f"B{b}-T{t}-A{a}" for b, t, a in D.KERNEL_CASES])
def test_loss_kernel_matches_float64(B, T_, A):
    """Head gradients by fp64_truth.grad_vs_exact at TOL, each loss within max(TOL, 2 x the float32 torch evaluation's own error), the multipliers'
    recorded gradients against the magnitude of their terms, and their step as arithmetic: float64 Adam fed the block's OWN recorded gradient lands
    on the block's new value (fp64_truth's per-element bound), moments at 1e-5; alpha_sigma and its moments are bit-unchanged.  Both `retrace`
    values where T > 1; random `done` with one inside a trajectory; prob_b on both sides of the clip."""
    c = D.case(B, T_, A)
    for retrace in ((True, False) if T_ > 1 else (True,)):
        _check_case(c, retrace, f"B{B} T{T_} A{A} retrace={int(retrace)}")


def test_loss_kernel_stays_finite_where_float32_exp_overflows_and_clamps_at_the_floors():
    """eta = 1e-3: At / eta runs past 88, the reference's float32 exp(At / eta) is inf; the kernel is checked against the float64 truth only.
    `floor`: both stepped multipliers cross their floors and are clamped to them."""
    c = D.case(16, 8, 2, "hot")
    assert not np.isfinite(D.case_truth(c, True, torch.float32)["eta_loss"]), "float32 torch overflows here"
    stats, _ = _check_case(c, True, "hot", against_fp32=False)
    assert np.isfinite(stats).all()
    c = D.case(5, 4, 3, "floor")
    _, blk = _check_case(c, True, "floor")
    for j in range(2):
        assert blk[D.NAMES[j]]["value"] == float(c["floors"][j]), f"{D.NAMES[j]} is clamped to its floor"


def test_kernel_is_bit_identical_across_runs_and_rejects_bad_sizes():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    for B, T_, A in ((33, 8, 6), (128, 8, 18)):
        c = D.case(B, T_, A)
        r1, r2 = _run_kernel(c), _run_kernel(c)
        for k in r1[0]:
            assert r1[0][k].tobytes() == r2[0][k].tobytes(), (B, T_, A, k)
        assert r1[1].tobytes() == r2[1].tobytes() and r1[4].tobytes() == r2[4].tobytes()
    blk, hyper = ops.vmpo_block(), ops.vmpo_hyper(1e-3)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    for R, T_, A in ((1025, 1, 2), (1032, 8, 2), (20, 3, 2), (4, 1, 1), (4, 1, 65), (4, 0, 2)):  # over the cap, R % T != 0, A < 2, A over its cap of 64, T < 1
        g_la, g_q, stats = z(R, A).fill_(-7.0), z(R, A).fill_(-7.0), z(11).fill_(-7.0)
        with pytest.raises(JhError, match="bad argument"):
            ops.mpo_loss_discrete(*[z(R, A) for _ in range(6)], *[z(R) for _ in range(4)], T_, blk, hyper, 0.99, stats=stats, out=(g_la, g_q))
        torch.cuda.synchronize()
        assert bool((g_la == -7.0).all()) and bool((g_q == -7.0).all()) and bool((stats == -7.0).all()), "nothing was launched"
    assert npy(blk).tobytes() == npy(ops.vmpo_block()).tobytes(), "a refused call leaves the block alone"


# ---------------------------------------------------------------------------------------------- online(s), online(s'), target(s)
def _policy_net(rows, S=4, A=3, H=64, seed=0):
    from jorldy_amd import ops
    from jorldy_amd.core.network import Network

    torch.manual_seed(seed)
    net = ops.RainbowNet(S, A, 1, H, "mlp", rows, "cuda:0", kind="pi")
    net.import_state(Network("discrete_policy", S, A, D_hidden=H, head="mlp").state_dict())
    tgt = Network("discrete_policy", S, A, D_hidden=H, head="mlp").state_dict()
    net.import_state({k: v + 0.1 * torch.randn_like(v) for k, v in tgt.items()}, net.target)
    with torch.no_grad():
        net.params.add_(0.1 * torch.randn_like(net.params))  # the policy gain is 0.01: move the last layer away from ~0
    return net


@pytest.mark.parametrize("rows", [1, 20, 264])
def test_learn_forward_p_equals_three_forwards_bit_for_bit_and_backward_continues(rows):
    S, A = 4, 3
    net = _policy_net(rows)
    x = torch.randn(2 * rows, S, device="cuda")
    out = torch.full((3, rows, A, 1), -7.0, device="cuda")
    net.learn_forward_p(x, rows, None, out)
    torch.cuda.synchronize()
    g = (torch.randn(rows, A, device="cuda") / rows).contiguous()
    net.backward(g)
    torch.cuda.synchronize()
    grads_p = net.export_state(net.grads)  # the parameters' segments (the bucket's alignment padding between them is nobody's)
    sep = [net.forward(x[:rows].contiguous(), 0).clone(), net.forward(x[rows:].contiguous(), 0).clone(), net.forward(x[:rows].contiguous(), 1).clone()]
    torch.cuda.synchronize()
    for i, what in enumerate(("online(state)", "online(next_state)", "target(state)")):
        assert torch.equal(out[i], sep[i]), what
    assert not torch.equal(out[0], out[2]), "the target differs from the online net here"
    out2 = torch.empty(3, rows, A, 1, device="cuda")
    net.grads.fill_(-3.0)
    net.learn_forward(x, rows, None, out2)
    net.backward(g)
    torch.cuda.synchronize()
    assert torch.equal(out2[0], out[0]) and torch.equal(out2[1], out[1])
    for k, v in net.export_state(net.grads).items():
        assert torch.equal(v, grads_p[k]) and float(v.abs().max()) > 0, f"{k}: the backward after learn_forward_p equals the backward after learn_forward on the same online rows"


def test_learn_forward_p_refuses_a_noisy_network_and_too_many_rows():
    from jorldy_amd import _lib as L
    from jorldy_amd import ops

    nat = ops.RainbowNet(4, 3, 11, 32, "mlp", 8, "cuda:0", kind="rainbow")
    with pytest.raises(L.JhError):
        nat.learn_forward_p(torch.zeros(16, 4, device="cuda"), 8, torch.zeros(3, nat.noise_len, device="cuda"), torch.empty(3, 8, 3, 11, device="cuda"))
    net = _policy_net(8)
    with pytest.raises(L.JhError):
        net.learn_forward_p(torch.zeros(18, 4, device="cuda"), 9, None, torch.empty(3, 9, 3, 1, device="cuda"))
    assert net.hyper_ptr() != 0


# ---------------------------------------------------------------------------------------------- the agent against the fixtures
def _agent_for(fx, **over):
    from jorldy_amd.core.agent import Agent

    kw = fx.agent_kwargs()
    kw.update(device="cuda")
    kw.update(over)
    agent = Agent("mpo", **kw)
    for n in D.NETS:
        getattr(agent, n).load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx.sd0(n).items()})
    agent.memory.first_store = False
    return agent


def _grads(net):
    return {k: npy(v) for k, v in net.export_state(net.grads).items()}


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name):
    """Every learn of the fixture on ONE agent with the recorded numpy seed (the first eager, the second -- mpo_discrete -- continues from the
    first's end with the multipliers after ONE step, the one-step lag): the same sampled rows; the six network outputs (rtol and atol 1e-5, the
    M-DQN fixture test's); the four losses and every result key (rtol 1e-5); the head gradients and both nets' clipped parameter gradients (1e-5 of
    the tensor's largest entry); the multipliers after their step (fp64_truth's per-element bound around the reference's value), their moments
    (2e-5); end weights within the caps of the other agents' fixture tests (at most 0.5 % further than 2e-5 from the reference's, the worst within
    2.1 lr).  Then a second agent runs the same through process(): the same bits, and target nets equal to their online nets."""
    fx = D.load_fixture(name)
    agent = _agent_for(fx)
    rows = fx.replay()
    agent.memory.store(rows)
    np.random.seed(fx.np_seed)
    R, A = fx.R, fx.A
    result = None
    for k in range(fx.learns):
        rec = fx.learn(k)
        mult_before = agent.multipliers()
        result = agent.learn()
        torch.cuda.synchronize()
        st = agent._static
        assert tuple(result) == D.STATS
        assert np.array_equal(npy(st["idx"]), rec["idx"]), "other rows were sampled"
        if k == 0:
            assert [mult_before[n]["value"] for n in D.NAMES] == [float(rec[f"mult0/{n}"]) for n in D.NAMES]
        la, lq = npy(st["la"]).reshape(3, R, A), npy(st["lq"]).reshape(3, R, A)
        for ours, key in ((la[0], "la"), (la[1], "la_next"), (la[2], "la_old"), (lq[0], "q"), (lq[1], "qt"), (lq[2], "qt_next")):
            np.testing.assert_allclose(ours, rec[key], rtol=1e-5, atol=1e-5, err_msg=f"l{k} {key}")
        for key in D.STATS:
            print(f"{name} l{k} {key}: ours {result[key]!r} reference {float(rec['result/' + key])!r}")
        for key in ("actor_loss", "critic_loss", "eta_loss", "alpha_loss", "min_Q", "max_Q", "min_At", "max_At"):
            np.testing.assert_allclose(result[key], float(rec[f"result/{key}"]), rtol=1e-5, err_msg=f"l{k} {key}")
        for ours, key in ((st["g_la"], "d_la"), (st["g_q"], "d_q")):
            margins.leq(float(np.abs(npy(ours) - rec[key]).max()) / float(np.abs(rec[key]).max()), 1e-5, f"l{k} {key}: max |diff| / the tensor's largest entry")
        blk = agent.multipliers()
        for j, n in enumerate(D.NAMES):
            x0, w = float(rec[f"mult0/{n}"]), float(rec[f"mult1/{n}"])
            margins.leq(abs(result[n] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * fx.lr, f"l{k} {n} after its step")
            assert blk[n]["value"] == result[n] and blk[n]["has_state"] == bool(int(rec[f"mult1/{n}/has_state"]))
            if blk[n]["has_state"]:
                np.testing.assert_allclose(blk[n]["m"], float(rec[f"mult1/{n}/exp_avg"]), rtol=2e-5, atol=1e-9, err_msg=f"l{k} {n} exp_avg")
                np.testing.assert_allclose(blk[n]["v"], float(rec[f"mult1/{n}/exp_avg_sq"]), rtol=2e-5, err_msg=f"l{k} {n} exp_avg_sq")
        assert agent._adam_steps == k + 1
        for label, net, view in (("actor", agent._actor, agent.actor), ("critic", agent._critic, agent.critic)):
            for key, g in _grads(net).items():  # the bucket holds the clipped gradient after the optimizer step
                ref = rec[f"grad_clip/{label}/{key}"]
                coef = min(1.0, fx.clip / (float(rec[f"grad_raw_norm/{label}"]) + 1e-6))
                scale = float(rec[f"grad_raw_absmax/{label}/{key}"]) * coef
                margins.leq(float(np.abs(fx.thin(g) - ref).max()) / scale, 1e-5, f"l{k} clipped d(loss)/d {label}.{key}: max |diff| / the tensor's largest entry")
            tot = bad = 0
            worst = 0.0
            for key, v in view.state_dict().items():
                dd = np.abs(fx.thin(npy(v)) - rec[f"sd1/{label}/{key}"])
                tot += dd.size
                bad += int((dd > 2e-5).sum())
                worst = max(worst, float(dd.max()) / fx.lr)
            margins.leq(bad / tot, 0.005, f"l{k} {label}: fraction of weights further than 2e-5 from the reference's")
            margins.leq(worst, 2.1, f"l{k} {label}: worst weight difference / lr vs the possible travel")
    if name == "mpo_td":
        assert result["eta"] == float(np.float32(fx.floors[0])), "the first step of eta is clamped to its floor"
    if name == "mpo_discrete":
        assert float(fx.learn(1)["mult0/eta"]) != fx.mult[0], "learn 1 starts from the multipliers after learn 0's step"
    # the same through process(): store, `learns` learns, hard target update
    other = _agent_for(fx)
    np.random.seed(fx.np_seed)
    res2 = other.process(rows, 1)
    torch.cuda.synchronize()
    assert res2 == result
    for a, b in ((agent._actor, other._actor), (agent._critic, other._critic)):
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert torch.equal(b.target, b.params) and not torch.equal(a.target, a.params), "process() ends with the hard copies of both nets"
    assert torch.equal(agent._mult, other._mult)


# ---------------------------------------------------------------------------------------------- graph replay, checkpoints
def _state(agent):
    return torch.cat([t for n in (agent._actor, agent._critic) for t in (n.params, n.target, n.m, n.v)] + [agent._mult]).clone()


def _small_agent(**over):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=4, action_size=3, hidden_size=32, optim_config={"name": "adam", "lr": 1e-3}, buffer_size=256, batch_size=6, start_train_step=0, n_epoch=3,
              n_step=4, run_step=40, lr_decay=True, eta=2.0, alpha_mu=0.5, device="cuda")
    kw.update(over)
    torch.manual_seed(5)
    agent = Agent("mpo", **kw)
    agent.memory.first_store = False
    return agent


def _rows(call, n=8, T=4, S=4, A=3):
    return D.replay(100 + call, n, T, S, A, done_rows=(1, 2))


def test_graph_replay_equals_eager_bit_for_bit_and_follows_the_learning_rate():
    """Three process() calls of three learns each, cosine decay over 40 steps: the first learn runs eagerly, the second is captured, seven are
    replayed.  Same bits as an agent that never captures -- weights, targets, moments, multipliers, results --, so the replayed graph reads the
    decayed learning rate (both nets' and, through the actor's block, the multipliers') and the multipliers of the learn before."""
    agents = [_small_agent(use_graph=g) for g in (True, False)]
    assert torch.equal(_state(agents[0]), _state(agents[1])), "one torch.manual_seed, the same initial weights"
    for call in range(3):
        res = []
        for a in agents:
            np.random.seed(7 + call)
            res.append(a.process(_rows(call), 10 * (call + 1)))
        torch.cuda.synchronize()
        assert res[0] == res[1] and set(res[0]) == set(D.STATS), call
        assert torch.equal(_state(agents[0]), _state(agents[1])), call
    assert agents[0]._graph is not None and agents[1]._graph is None and agents[0].num_learn == 9
    assert agents[0]._lr_now == pytest.approx(1e-3 * np.cos(0.5 * np.pi * 30 / 40))
    frozen = _small_agent(use_graph=True, lr_decay=False)
    for call in range(3):
        np.random.seed(7 + call)
        frozen.process(_rows(call), 10 * (call + 1))
    torch.cuda.synchronize()
    assert not torch.equal(_state(frozen), _state(agents[0])), "the decay is visible in the weights"
    assert frozen.eta != agents[0].eta, "and in the multipliers, which step with the actor's learning rate"


def test_save_load_roundtrip_in_the_reference_format(tmp_path):
    from jorldy_amd.core.network import Network

    agent = _small_agent()
    for call in range(2):
        np.random.seed(call)
        agent.process(_rows(call), 10 * (call + 1))
    agent.save(str(tmp_path))
    ck = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert set(ck) == {"actor", "critic", "actor_optimizer", "critic_optimizer"}
    assert list(ck["actor"]) == ["head.l.weight", "head.l.bias", "l.weight", "l.bias", "pi.weight", "pi.bias"] and list(ck["critic"])[-2:] == ["q.weight", "q.bias"]
    # the file loads into torch modules of the reference's shapes and torch.optim.Adam over the actor's parameters followed by the three scalars
    actor, critic = Network("discrete_policy", 4, 3, D_hidden=32, head="mlp"), Network("discrete_q_network", 4, 3, D_hidden=32, head="mlp")
    actor.load_state_dict(ck["actor"])
    critic.load_state_dict(ck["critic"])
    scalars = [torch.nn.Parameter(torch.tensor(1.0)) for _ in range(3)]
    opt_a, opt_c = torch.optim.Adam(list(actor.parameters()) + scalars, lr=1e-3), torch.optim.Adam(critic.parameters(), lr=1e-3)
    opt_a.load_state_dict(ck["actor_optimizer"])
    opt_c.load_state_dict(ck["critic_optimizer"])
    blk = agent.multipliers()
    assert float(opt_a.state[scalars[0]]["exp_avg"]) == np.float32(blk["eta"]["m"]) and float(opt_a.state[scalars[1]]["exp_avg_sq"]) == np.float32(blk["alpha_mu"]["v"])
    assert scalars[2] not in opt_a.state, "alpha_sigma never took a step: no optimizer state, as in torch"
    assert float(opt_a.state[scalars[0]]["step"]) == 6.0 == float(opt_c.state[next(iter(critic.parameters()))]["step"])
    assert opt_a.param_groups[0]["lr"] == pytest.approx(agent._lr_now)
    other = _small_agent(eta=2.0, alpha_mu=0.5)
    other.load(str(tmp_path))
    torch.cuda.synchronize()
    for a, b in ((agent._actor, other._actor), (agent._critic, other._critic)):
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert torch.equal(b.target, b.params), "targets equal their online nets after load()"
    mo = other.multipliers()
    for n in ("eta", "alpha_mu"):
        assert (mo[n]["m"], mo[n]["v"], mo[n]["has_state"]) == (blk[n]["m"], blk[n]["v"], True)
    assert mo["eta"]["value"] == 2.0 and mo["alpha_mu"]["value"] == 0.5, "the multipliers' VALUES are not part of the reference's checkpoint"
    assert other._adam_steps == 6 and other._lr_now == pytest.approx(agent._lr_now)


def test_save_full_load_full_resumes_bit_for_bit(tmp_path):
    agent = _small_agent()
    for call in range(2):
        np.random.seed(call)
        agent.process(_rows(call), 10 * (call + 1))
    agent.save_full(str(tmp_path))
    resumed = _small_agent(eta=1.0, alpha_mu=1.0)
    resumed.load_full(str(tmp_path))
    torch.cuda.synchronize()
    assert torch.equal(_state(agent), _state(resumed)) and resumed.memory.size == agent.memory.size == 16
    out = []
    for a in (agent, resumed):
        np.random.seed(11)
        out.append([a.process(_rows(call), 10 * (call + 1)) for call in (2, 3)])
    torch.cuda.synchronize()
    assert out[0] == out[1] and torch.equal(_state(agent), _state(resumed))


def test_sync_carries_the_actor_only():
    a, b = _small_agent(), _small_agent()
    with torch.no_grad():
        a._actor.params.add_(0.01)
        a._critic.params.add_(0.01)
    payload = a.sync_out()
    assert set(payload) == {"weights"} and list(payload["weights"])[-1] == "pi.bias" and all(v.device.type == "cpu" for v in payload["weights"].values())
    before = b._critic.params.clone()
    b.sync_in(payload["weights"])
    for k, v in a.actor.state_dict().items():
        assert torch.equal(v, b.actor.state_dict()[k]), k
    assert torch.equal(b._critic.params, before) and not torch.equal(b._actor.target, b._actor.params), "the critic and the targets are not part of a sync"


# ---------------------------------------------------------------------------------------------- the reference's configurations, acting
CONFIGS = [("cartpole", dict(state_size=4, action_size=2, batch_size=64, n_step=4, n_epoch=16, eps_eta=0.02, eps_alpha_mu=0.01, eps_alpha_sigma=0.01,
                             optim_config={"name": "adam", "lr": 2.5e-4})),
           ("mountaincar", dict(state_size=2, action_size=3, batch_size=128, n_step=8, n_epoch=64, optim_config={"name": "adam", "lr": 5e-4})),
           ("pong_mlagent", dict(state_size=8, action_size=3, batch_size=64, n_step=8, n_epoch=64, critic_loss_type="1step_TD", optim_config={"name": "adam", "lr": 2.5e-4}))]


@pytest.mark.parametrize("label,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_reference_config_constructs_and_learns_once(label, kw):
    """The discrete MLP configurations under config/mpo/ at their shapes (mountaincar is the 1024-row cap): construction, one process() with its
    n_epoch learns, finite results, moved weights, targets equal to their online nets."""
    from jorldy_amd.core.agent import Agent

    agent = Agent("mpo", device="cuda", actor="discrete_policy", critic="discrete_q_network", start_train_step=0, run_step=100000, **kw)
    agent.memory.first_store = False
    T_ = agent.n_step
    assert T_ == (1 if kw.get("critic_loss_type") == "1step_TD" else kw["n_step"])
    w0 = _state(agent)
    np.random.seed(0)
    result = agent.process(D.replay(3, kw["batch_size"], T_, kw["state_size"], kw["action_size"], done_rows=(0, 5)), 1)
    torch.cuda.synchronize()
    assert tuple(result) == D.STATS and all(np.isfinite(v) for v in result.values()), result
    assert agent.num_learn == kw["n_epoch"] and not torch.equal(w0, _state(agent))
    assert torch.equal(agent._actor.target, agent._actor.params) and torch.equal(agent._critic.target, agent._critic.params)
    assert result["alpha_sigma"] == 1.0 and result["eta"] != 1.0


@pytest.mark.parametrize("rows", [1, 5])
def test_act_returns_each_rows_own_probability(rows):
    agent = _small_agent()
    with torch.no_grad():
        agent._actor.params.add_(0.3 * torch.randn_like(agent._actor.params))  # away from the near-uniform initial policy
    x = np.random.RandomState(rows).randn(rows, 4).astype(np.float32)
    pi = torch.softmax(agent.actor(agent.as_tensor(x)), -1).cpu().numpy()
    assert np.unique(pi.round(4), axis=0).shape[0] == rows, "the rows' policies differ"
    for training in (True, False):
        torch.manual_seed(1)
        out = agent.act(x, training)
        assert set(out) == {"action", "prob"} and out["action"].shape == out["prob"].shape == (rows, 1) and out["action"].dtype == np.int64
        assert np.array_equal(out["prob"][:, 0], pi[np.arange(rows), out["action"][:, 0]]), "each row's own pi[action]"
        if not training:
            assert np.array_equal(out["action"][:, 0], pi.argmax(-1))
    if rows == 1:
        assert out["prob"][0, 0] == np.take(pi, out["action"])[0, 0], "identical to the reference's np.take at one row"


# ---------------------------------------------------------------------------------------------- learning curve
def _hip_curve(seed, bin_):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    c = D.CURVE_CONFIG
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = Agent("mpo", run_step=c["run_step"], device="cuda", **c["agent"])
    agent.memory.first_store = False
    env = ops.CartPoleVec(1, seed=1000 + seed)
    out, acc = [], 0.0
    for step in range(1, c["steps"] + 1):
        state = env.obs().copy()  # the window keeps it for n_step steps
        a = agent.act(state, True)
        nxt, rew, done = env.step(a["action"].reshape(-1))
        tr = {"state": state, "next_state": np.array(nxt, np.float32), "reward": np.asarray(rew, np.float64).reshape(1, 1), "done": np.asarray(done).reshape(1, 1).astype(bool)}
        tr.update(a)
        tr = agent.interact_callback(tr)
        if tr:
            agent.process([tr], step)
        acc += float(np.asarray(rew).reshape(-1)[0])
        if step % bin_ == 0:
            out.append(acc / bin_)
            acc = 0.0
    return out


def test_cartpole_learning_curve_tracks_the_real_reference():
    """One seed at the JSON's configuration, single mode on ops.CartPoleVec, against the three curves of the UNMODIFIED reference agent on the
    oracle's CartPole (tests/golden/curves_reference_mpo.json, tools/gen_golden_mpo.py).  The last tenth's mean reward per step r is compared as
    the mean episode length it stands for -- the reward is 0.1 per step and -1 at an episode end, so r = 0.1 - 1.1 / L exactly --, which must
    lie within the band of the reference's three seeds widened by the factor 2 of tests/test_vmpo_gpu.py's curve test (episode length is what that
    factor was set for); and the curve learns: its last tenth lies above its first."""
    with open(os.path.join(D.GOLDEN, "curves_reference_mpo.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_mpo.py --only curves"
    ref = fx["mpo_cartpole"]["reference"]
    hip = _hip_curve(1, fx["bin"])
    length = lambda r: 1.1 / (0.1 - r)
    r_len = [length(D.curve_tenths(c)[1]) for c in ref]
    first, last = D.curve_tenths(hip)
    g_len = length(last)
    margins.record(max(g_len / max(r_len), min(r_len) / g_len), 2.0, "mpo: end of the HIP curve vs the band of the reference's three seeds, as a factor")
    with open(os.path.join(os.path.dirname(margins.dump()), "learning_curve_mpo_cartpole.json"), "w") as f:
        json.dump({"config": fx["config"], "metric": fx["metric"], "hip": hip, "reference": ref, "hip_end_length": g_len, "reference_end_lengths": r_len}, f)
    print(f"MPO CartPole: HIP first / last tenth {first:.4f} / {last:.4f} (episode length {g_len:.1f}); reference end lengths {r_len}")
    assert np.isfinite(hip).all()
    assert last > first, "the curve learns"
    assert 0.5 * min(r_len) <= g_len <= 2.0 * max(r_len)
