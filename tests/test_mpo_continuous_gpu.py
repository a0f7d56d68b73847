"""Continuous MPO's kernels on the GPU against the float64 truth of tests/mpo_cont_truth.py at the smallest shapes that can still go wrong:
jh_mpo_sample (one row, ragged wavefronts, several workgroups, the +-5 clamp) and jh_mpo_loss_continuous (the same shapes, both caps at once, the
A cap, the degenerate E-step at N = 1, saturated stored actions, clamped raw mu, eta = 1e-3 where the reference's float32 overflows, a trajectory
whose every step is done, all three multipliers crossing their floors), the multipliers' device-side Adam step as arithmetic, determinism and
argument checks; the critic over sampled actions against torch float64 and bit for bit against the forward on repeated states, its fit step; the
agent: initial weights from one seed, one learn as the composition of its parts, graph replay against eager bit for bit under injected noise,
checkpoints, act(), the reference's configurations, and every learn of the three fixtures of tools/gen_golden_mpo_continuous.py."""
import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import mpo_cont_truth as D
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_mpo_gpu.py's


# ---------------------------------------------------------------------------------------------- the sampling kernel
@pytest.mark.parametrize("R,N,A", [(r, n, a) for r, _, n, a in D.SAMPLE_CASES], ids=[f"R{r}-N{n}-A{a}" for r, _, n, a in D.SAMPLE_CASES])
def test_sample_kernel_matches_float64(R, N, A):
    """z and tanh(z) of both policies within max(TOL, 2 x the float32 torch evaluation's own error) of the float64 truth, relative to the tensor's
    largest entry; every output element written, nothing around them."""
    from jorldy_amd import ops

    c = D.sample_case(R, N, A)
    t64, t32 = D.sample(**c), D.sample_torch(**c)
    pad = 64
    z = torch.full((2 * N * R * A + 2 * pad,), -7.0, device="cuda")
    a = torch.full((2 * N * R * A + 2 * pad,), -7.0, device="cuda")
    out = ops.mpo_sample(f32(c["head_next"]), f32(c["head_old"]), f32(c["eps"]), out=(z[pad:-pad].view(2, N, R, A), a[pad:-pad].view(2, N, R, A)))
    torch.cuda.synchronize()
    for ours, key in zip(out, ("zn", "zt_add", "a_next", "a_add")):
        assert tuple(ours.shape) == (N, R, A) and np.isfinite(npy(ours)).all()
        T.grad_vs_exact(npy(ours), t64[key], t32[key], TOL, f"R{R} N{N} A{A} {key}")
    for buf in (z, a):
        assert bool((buf[:pad] == -7.0).all()) and bool((buf[-pad:] == -7.0).all()), "nothing is written outside [2][N][R][A]"
    assert np.abs(npy(out[2])).max() <= 1.0 and np.abs(npy(out[3])).max() <= 1.0


# ---------------------------------------------------------------------------------------------- the loss kernel
def _run_kernel(c, retrace=True):
    """-> (grads {"head", "q"}, stats [11], block after (ops.vmpo_block_read), raw block before, raw block after)"""
    from jorldy_amd import ops

    blk = ops.vmpo_block(*[float(x) for x in c["mult"]], *[float(x) for x in c["floors"]], *c["eps"], m=c["m"], v=c["v"], has_state=(True, True, True))
    blk[:3] = f32(c["mult"])  # exactly the case's values
    before = npy(blk).copy()
    hyper = ops.vmpo_hyper(D.LR, D.BETAS[0], D.BETAS[1], D.ADAM_EPS, D.STEP0)
    g_h, g_q, stats = ops.mpo_loss_continuous(*[f32(v) for v in D.case_args(c)], c["T"], blk, hyper, c["gamma"], retrace=retrace)
    torch.cuda.synchronize()
    return {"head": npy(g_h), "q": npy(g_q)}, npy(stats).copy(), ops.vmpo_block_read(blk), before, npy(blk).copy()


def _scalar(ours, exact, ref32, what):
    """tests/test_mpo_gpu.py's rule: |ours - exact| / |exact| <= max(TOL, 2 x the float32 reference's own error); a float32 reference that is
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
    A = c["A"]
    for k, g in grads.items():
        assert np.isfinite(g).all(), f"{what}: d {k}"
        T.grad_vs_exact(g, t64["grads"][k], t32["grads"][k] if t32 else None, TOL, f"{what} d(loss)/d {k}")
    clamped = np.abs(t64["mu_raw"]) > 5.0
    assert clamped.any() and not grads["head"][:, :A][clamped].any(), "no gradient into a raw mu outside [-5, 5]"
    for j, key in enumerate(("actor", "critic", "eta_loss", "alpha_loss")):
        assert np.isfinite(stats[j]), f"{what}: {key}"
        _scalar(stats[j], t64[key], t32[key] if t32 else float("nan"), f"{what} {key}")
    for j in range(3):
        n = D.NAMES[j]
        g = blk[n]["grad"]
        e_ref = abs(t32["mult_grads"][j] - t64["mult_grads"][j]) / t64["mult_scale"][j] if (t32 and np.isfinite(t32["mult_grads"][j])) else 0.0
        margins.leq(abs(g - t64["mult_grads"][j]) / t64["mult_scale"][j], max(TOL, 2.0 * e_ref), f"{what} d(loss)/d {n} against the magnitude of its terms")
        x0 = float(c["mult"][j])
        w, m, v = D.multiplier_step(x0, g, c["m"][j], c["v"][j], D.STEP0, D.LR, c["floors"][j], D.BETAS, D.ADAM_EPS)
        margins.leq(abs(blk[n]["value"] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * D.LR, f"{what} {n} after float64 Adam on OUR gradient")
        margins.leq(abs(blk[n]["m"] - m), 1e-5 * abs(m), f"{what} {n} exp_avg")
        margins.leq(abs(blk[n]["v"] - v), 1e-5 * abs(v), f"{what} {n} exp_avg_sq")
        assert blk[n]["has_state"] and stats[4 + j] == np.float32(blk[n]["value"]), f"all three multipliers step: {n}"
    assert raw0[9:15].tobytes() == raw1[9:15].tobytes(), "floors and thresholds are only read"
    # extrema: q is an input, exact.  At is a float64 value rounded once to float32; the truth's mean may differ from the kernel's in the last bits
    # of a double (summation order), so the two roundings differ by at most one float32 ulp (N = 1: At is exactly 0 on both sides)
    assert (stats[7], stats[8]) == (np.float32(t64["extrema"][0]), np.float32(t64["extrema"][1])) == (c["q"].min(), c["q"].max())
    for j in (2, 3):
        margins.leq(abs(float(stats[7 + j]) - t64["extrema"][j]), 2.0 ** -23 * abs(t64["extrema"][j]), f"{what} {'min' if j == 2 else 'max'} At within one float32 ulp")
    return stats, blk


@pytest.mark.parametrize("R,T_,N,A", D.LOSS_CASES, ids=[f"R{r}-T{t}-N{n}-A{a}" for r, t, n, a in D.LOSS_CASES])
def test_loss_kernel_matches_float64(R, T_, N, A):
    """Head gradients and d q by fp64_truth.grad_vs_exact at TOL, each loss within max(TOL, 2 x the float32 torch evaluation's own error), the three
    multipliers' recorded gradients against the magnitude of their terms, and their step as arithmetic: float64 Adam fed the block's OWN recorded
    gradient lands on the block's new value, moments at 1e-5.  Both `retrace` values where T > 1; every case has a clamped raw mu, saturated
    stored actions (R >= 3), a done inside a trajectory and prob_b on both sides of the clip."""
    c = D.case(R, T_, N, A)
    for retrace in ((True, False) if T_ > 1 else (True,)):
        _check_case(c, retrace, f"R{R} T{T_} N{N} A{A} retrace={int(retrace)}")


def test_loss_kernel_stays_finite_where_float32_overflows_handles_an_all_done_trajectory_and_clamps_at_the_floors():
    """eta = 1e-3: At / eta runs past 88, the reference's float32 exp(At / eta) is inf; the kernel is checked against the float64 truth alone.
    `alldone`: trajectory 0's targets are its rewards.  `floor`: all three stepped multipliers cross their floors and are clamped to them."""
    c = D.case(64, 4, 30, 3, "hot")
    assert not np.isfinite(D.case_truth(c, True, torch.float32)["eta_loss"]), "float32 torch overflows here"
    stats, _ = _check_case(c, True, "hot", against_fp32=False)
    assert np.isfinite(stats).all()
    _check_case(D.case(64, 4, 30, 3, "alldone"), True, "alldone")
    c = D.case(20, 4, 6, 3, "floor")
    _, blk = _check_case(c, True, "floor")
    for j in range(3):
        assert blk[D.NAMES[j]]["value"] == float(c["floors"][j]), f"{D.NAMES[j]} is clamped to its floor"


def test_kernels_are_bit_identical_across_runs_and_reject_bad_sizes():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    for R, T_, N, A in ((20, 4, 6, 3), (1024, 8, 8, 2)):
        c = D.case(R, T_, N, A)
        r1, r2 = _run_kernel(c), _run_kernel(c)
        for k in r1[0]:
            assert r1[0][k].tobytes() == r2[0][k].tobytes(), (R, T_, N, A, k)
        assert r1[1].tobytes() == r2[1].tobytes() and r1[4].tobytes() == r2[4].tobytes()
    blk, hyper = ops.vmpo_block(), ops.vmpo_hyper(1e-3)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    # R over its cap, N * R over its cap, R % T != 0, A over its cap, T < 1
    for R, T_, N, A in ((1025, 1, 1, 1), (1024, 8, 9, 1), (512, 8, 17, 2), (20, 3, 2, 2), (4, 1, 2, 9), (4, 0, 2, 2)):
        g_h, g_q, stats = z(R, 2 * A).fill_(-7.0), z(R).fill_(-7.0), z(11).fill_(-7.0)
        with pytest.raises(JhError, match="bad argument"):
            ops.mpo_loss_continuous(z(R, 2 * A), z(R, 2 * A), z(R), z(R), z(N, R), z(N, R), z(N, R, A), z(R, A), z(R), z(R), z(R), T_, blk, hyper, 0.99, stats=stats,
                                    out=(g_h, g_q))
        torch.cuda.synchronize()
        assert bool((g_h == -7.0).all()) and bool((g_q == -7.0).all()) and bool((stats == -7.0).all()), "nothing was launched"
    assert npy(blk).tobytes() == npy(ops.vmpo_block()).tobytes(), "a refused call leaves the block alone"
    for R, N, A in ((1025, 1, 1), (1024, 9, 1), (4, 2, 9)):
        out = (z(2, N, R, A).fill_(-7.0), z(2, N, R, A).fill_(-7.0))
        with pytest.raises(JhError, match="bad argument"):
            ops.mpo_sample(z(R, 2 * A), z(R, 2 * A), z(2, N, R, A), out=out)
        torch.cuda.synchronize()
        assert bool((out[0] == -7.0).all()) and bool((out[1] == -7.0).all())


# ---------------------------------------------------------------------------------------------- the critic over sampled actions
def _critic(S, A, H, max_batch, sampled_rows, seed=0):
    """An ops.ACNet with one critic, online and target weights from two float64 mirrors (tests/td3_truth.py's Critic) rounded to float32."""
    import td3_truth as TD
    from jorldy_amd import ops

    mirrors = []
    for s in (seed, seed + 100):
        torch.manual_seed(s)
        m = TD.Critic(S, A, H).double()
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 1:
                    p.add_(0.05 * torch.randn_like(p))
        T.round_to_fp32_(m)
        mirrors.append((m, T.as32(m)))
    nat = ops.ACNet(S, A, H, 1, max_batch, "cuda:0")
    nat.import_state(mirrors[0][1].state_dict(), "critic")
    nat.import_state(mirrors[1][1].state_dict(), "critic", "target")
    nat.reserve_sampled(sampled_rows)
    return nat, mirrors


@pytest.mark.parametrize("H", [32, 512])
@pytest.mark.parametrize("R,N", [(1, 1), (20, 6), (65, 2), (256, 30)])
def test_sampled_critic_forward_matches_float64_and_the_forward_on_repeated_states(R, N, H):
    """critic(which, x [R, S], actions [N, R, A]) -> q [N, R] against torch float64 on the same weights (fp64_truth.vs_exact at TOL), online and
    target; and the online one against critic_forward on the states repeated N times, which is what the reference runs (mpo.py:228-231)."""
    S, A = 4, 3
    nat, mirrors = _critic(S, A, H, N * R, N * R)
    g = torch.Generator().manual_seed(R + N)
    x, acts = torch.randn(R, S, generator=g), torch.tanh(torch.randn(N, R, A, generator=g))
    rep = x.unsqueeze(0).repeat_interleave(N, dim=0)
    for which, (m64, m32) in enumerate(mirrors):
        with torch.no_grad():
            q64, q32 = m64(rep.double(), acts.double()), m32(rep, acts)
        q = nat.critic_forward_sampled(x.cuda(), acts.cuda(), which)
        torch.cuda.synchronize()
        assert tuple(q.shape) == (N, R)
        T.vs_exact(q, q64.reshape(N, R), q32.reshape(N, R), TOL, f"R{R} N{N} H{H} sampled critic which={which}")
    plain = nat.critic_forward(rep.reshape(N * R, S).contiguous().cuda(), acts.reshape(N * R, A).contiguous().cuda(), 0)[0].view(N, R)
    q = nat.critic_forward_sampled(x.cuda(), acts.cuda(), 0)
    torch.cuda.synchronize()
    # e(a), l and q are the same tile-engine problems on the same N * R rows, and head.l(s) has one K chunk: the same bits
    assert torch.equal(q, plain), f"R{R} N{N} H{H}: sampled forward vs critic_forward on repeated states, max diff {float((q - plain).abs().max()):.3e}"


@pytest.mark.parametrize("R,N,H", [(20, 6, 32), (256, 30, 512)])
def test_mpo_forward_equals_the_four_separate_forwards_and_refuses_what_does_not_fit(R, N, H):
    from jorldy_amd._lib import JhError

    S, A = 4, 3
    nat, _ = _critic(S, A, H, R, N * R, seed=3)
    g = torch.Generator().manual_seed(7)
    x_all, act = torch.randn(2 * R, S, generator=g).cuda(), torch.tanh(torch.randn(R, A, generator=g)).cuda()
    a_next, a_add = torch.tanh(torch.randn(N, R, A, generator=g)).cuda(), torch.tanh(torch.randn(N, R, A, generator=g)).cuda()
    xs, xn = x_all[:R].contiguous(), x_all[R:].contiguous()
    sep = (nat.critic_forward(xs, act, 0)[0].clone(), nat.critic_forward(xs, act, 1)[0].clone(), nat.critic_forward_sampled(xn, a_next, 1).clone(),
           nat.critic_forward_sampled(xs, a_add, 1).clone())
    out = nat.mpo_forward(x_all, act, a_next, a_add)
    torch.cuda.synchronize()
    for ours, ref, what in zip(out, sep, ("online(s, a)", "target(s, a)", "target(s', a_next)", "target(s, a_add)")):
        margins.leq(float((ours.reshape(ref.shape) - ref).abs().max()), 1e-6 * float(ref.abs().max()) + 1e-7, f"R{R} N{N} H{H} mpo_forward {what}")
    assert not torch.equal(out[0], out[1]), "the target differs from the online critic here"
    q = torch.full((N + 1, R), -7.0, device="cuda")
    with pytest.raises(JhError, match="bad argument"):
        nat.critic_forward_sampled(xs, torch.zeros(N + 1, R, A, device="cuda"), 0, out=q)  # over the reserved rows
    with pytest.raises(JhError, match="bad argument"):
        nat.critic_forward_sampled(torch.zeros(R + 1, S, device="cuda"), torch.zeros(1, R + 1, A, device="cuda"), 0)  # R over max_batch
    torch.cuda.synchronize()
    assert bool((q == -7.0).all()), "nothing was launched"


@pytest.mark.parametrize("R,H", [(20, 32), (256, 512)])
def test_critic_fit_matches_float64(R, H):
    """mpo_forward, then critic_fit with a caller's dq: the clipped gradient left in the bucket against float64 autograd + clip_grad_norm_
    (fp64_truth.vs_exact at TOL per tensor), the Adam step as arithmetic on OUR gradient (fp64_truth.check_first_step_from_our_gradient), the
    moments at 1e-5; the target bucket and the actor's buckets are not written."""
    S, A, N, lr, clip = 4, 3, 2, 1e-3, 1.0
    nat, mirrors = _critic(S, A, H, R, N * R, seed=5)
    nat.set_hyper("critic", lr, 0.9, 0.999, 1e-8, 0)
    g = torch.Generator().manual_seed(11)
    x_all, act = torch.randn(2 * R, S, generator=g), torch.tanh(torch.randn(R, A, generator=g))
    a_s = torch.tanh(torch.randn(2, N, R, A, generator=g))
    dq = torch.randn(R, generator=g) * 2.0  # d(loss)/d(q) of a sum, not of a mean: a gradient norm well above the clip
    w0 = {k: v.clone() for k, v in nat.export_state("critic").items()}
    tgt0, actor0 = nat.critics["target"].clone(), {k: v.clone() for k, v in nat.actor.items()}
    nat.mpo_forward(x_all.cuda(), act.cuda(), a_s[0].cuda(), a_s[1].cuda())
    nat.critic_fit(x_all[:R].contiguous().cuda(), act.cuda(), dq.cuda(), clip)
    torch.cuda.synchronize()
    ref = {}
    for dt, m in ((torch.float64, mirrors[0][0]), (torch.float32, mirrors[0][1])):
        for p in m.parameters():
            p.grad = None
        (m(x_all[:R].to(dt), act.to(dt)).reshape(-1) * dq.to(dt)).sum().backward()
        norm = float(torch.nn.utils.clip_grad_norm_(m.parameters(), clip))
        ref[dt] = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    assert norm > 2.0 * clip, "the clip is active"
    ours = nat.export_state("critic", "grads")
    for k in ref[torch.float64]:
        T.vs_exact(ours[k], ref[torch.float64][k], ref[torch.float32][k], TOL, f"R{R} H{H} clipped d(loss)/d critic.{k}")
    T.check_first_step_from_our_gradient(w0, ours, nat.export_state("critic"), lambda ps: torch.optim.Adam(ps, lr=lr), lr, f"R{R} H{H} critic fit")
    for kind, f in (("m", lambda gr: 0.1 * gr), ("v", lambda gr: 0.001 * gr * gr)):
        for k, v in nat.export_state("critic", kind).items():
            exact = f(ours[k].double().cpu())
            margins.leq(float((v.double().cpu() - exact).abs().max()), 1e-5 * float(exact.abs().max()) + 1e-30, f"R{R} H{H} critic.{k} {kind}")
    assert torch.equal(nat.critics["target"], tgt0) and all(torch.equal(nat.actor[k], actor0[k]) for k in actor0)


# ---------------------------------------------------------------------------------------------- the agent
def _small_agent(seed=5, **over):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=4, action_size=3, hidden_size=32, actor="continuous_policy", critic="continuous_q_network", optim_config={"name": "adam", "lr": 1e-3},
              buffer_size=256, batch_size=5, start_train_step=0, n_epoch=3, n_step=4, num_sample=6, run_step=40, lr_decay=True, eta=2.0, alpha_mu=0.5, alpha_sigma=0.7,
              device="cuda")
    kw.update(over)
    torch.manual_seed(seed)
    agent = Agent("mpo", **kw)
    agent.memory.first_store = False
    return agent


def _rows(call, n=8, T=4, S=4, A=3):
    return D.replay(100 + call, n, T, S, A, done_rows=(1, 2))


def _state(agent):
    return torch.cat([t for n in (agent._actor, agent._critic) for t in (n.params, n.target, n.m, n.v)] + [agent._mult]).clone()


def _eps(agent, call):
    R = agent.batch_size * agent.n_step
    return np.random.RandomState(900 + call).randn(2, agent.num_sample, R, agent.action_size).astype(np.float32)


def test_agent_is_the_sibling_class_with_the_reference_initial_weights_from_one_seed():
    from jorldy_amd.core.agent.mpo import MPO, MPOContinuous
    from jorldy_amd.core.network import Network

    agent = _small_agent(seed=9)
    assert type(agent) is MPOContinuous and isinstance(agent, MPO) and agent.action_type == "continuous" and agent.n_step == 4
    torch.manual_seed(9)
    mods = [Network(n, 4, 3, D_hidden=32, head="mlp") for n in ("continuous_policy", "continuous_policy", "continuous_q_network", "continuous_q_network")]
    for view, tview, mod in ((agent.actor, agent.target_actor, mods[0]), (agent.critic, agent.target_critic, mods[2])):
        sd = view.state_dict()
        assert list(sd) == list(mod.state_dict())
        for k, v in mod.state_dict().items():
            assert torch.equal(sd[k].cpu(), v) and torch.equal(tview.state_dict()[k].cpu(), v), k
    assert list(agent.actor.state_dict())[-4:] == ["mu.weight", "mu.bias", "log_std.weight", "log_std.bias"] and list(agent.critic.state_dict())[2] == "e.weight"


def test_one_learn_is_the_composition_of_the_forwards_the_sampling_and_the_float64_loss():
    """An eager learn() with injected normals, read back from its static buffers: the actor's three raw heads and the critic's four outputs against
    a second agent with the same seed (untouched weights) running them one by one; z and tanh(z) against the float64 sampling; the losses, both
    head gradients and all three multipliers' steps against the float64 loss on those buffers; then both networks have stepped."""
    agent, other = _small_agent(use_graph=False), _small_agent(use_graph=False)
    with torch.no_grad():  # away from the near-zero initial policy head, the target a little away from the online net
        for a in (agent, other):
            g = torch.Generator(device="cuda").manual_seed(3)
            a._actor.params.add_(0.2 * torch.randn(a._actor.params.shape, device="cuda", generator=g))
            a._actor.target.add_(0.2 * torch.randn(a._actor.params.shape, device="cuda", generator=g))
            a._critic.target.add_(0.05 * torch.randn(a._critic.target.shape, device="cuda", generator=g))
    w0 = _state(agent)
    assert torch.equal(w0, _state(other))
    agent.memory.store(_rows(0))
    np.random.seed(4)
    agent._noise_inject = _eps(agent, 0)
    mult0 = agent.multipliers()
    result = agent.learn()
    torch.cuda.synchronize()
    st, R, A, N = agent._static, 20, 3, 6
    la = npy(st["la"]).reshape(3, R, 2 * A)
    xs, xn = st["x_all"][:R].contiguous(), st["x_all"][R:].contiguous()
    act = st["tr"]["action"].reshape(R, A).contiguous()
    for i, (x, which) in enumerate(((xs, 0), (xn, 0), (xs, 1))):
        assert torch.equal(st["la"][i].view(R, 2 * A), other._actor.forward(x, which).view(R, 2 * A)), f"actor forward {i}"
    t = D.sample(la[1], la[2], npy(st["eps"]))
    for ours, key in ((st["z"][0], "zn"), (st["z"][1], "zt_add"), (st["a"][0], "a_next"), (st["a"][1], "a_add")):
        T.grad_vs_exact(npy(ours), t[key], None, TOL, f"agent {key}")
    cn = other._critic.nat
    sep = (cn.critic_forward(xs, act, 0)[0], cn.critic_forward(xs, act, 1)[0], cn.critic_forward_sampled(xn, st["a"][0].contiguous(), 1),
           cn.critic_forward_sampled(xs, st["a"][1].contiguous(), 1))
    for ours, ref, what in zip(st["lq"], sep, ("q", "qt_a", "qt_next", "qt_add")):
        margins.leq(float((ours.reshape(ref.shape) - ref).abs().max()), 1e-6 * float(ref.abs().max()) + 1e-7, f"agent {what}")
    tr = st["tr"]
    m0 = [mult0[n]["value"] for n in D.NAMES]
    t64 = D.loss(la[0], la[2], *[npy(v) for v in st["lq"]], npy(st["z"][1]), npy(act), npy(tr["reward"]), npy(tr["done"]), npy(tr["prob"]), 4, m0,
                 (agent.eps_eta, agent.eps_alpha_mu, agent.eps_alpha_sigma), agent.gamma, True)
    for key, ours in (("head", st["g_la"]), ("q", st["g_q"])):
        T.grad_vs_exact(npy(ours), t64["grads"][key], None, TOL, f"agent d(loss)/d {key}")
    for key, name in (("actor", "actor_loss"), ("critic", "critic_loss"), ("eta_loss", "eta_loss"), ("alpha_loss", "alpha_loss")):
        _scalar(result[name], t64[key], float("nan"), f"agent {name}")
    blk = agent.multipliers()
    for j, n in enumerate(D.NAMES):
        w, m, v = D.multiplier_step(m0[j], t64["mult_grads"][j], 0.0, 0.0, 0, 1e-3, 1e-8)
        margins.leq(abs(blk[n]["value"] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - m0[j]) + 1e-6 * 1e-3, f"agent {n} after its first step")
        assert blk[n]["has_state"] and result[n] == blk[n]["value"], n
    assert (c := t64["c"]).min() < 1.0 and (np.abs(npy(act)) == 1.0).any() and np.isfinite(list(result.values())).all() and tuple(result) == D.STATS
    for net in (agent._actor, agent._critic):
        assert float(net.grads.abs().max()) > 0 and float(net.m.abs().max()) > 0 and not torch.equal(net.params, net.target)
    assert agent._adam_steps == 1 and not torch.equal(_state(agent), w0)
    assert float(agent._critic.nat.actor["params"].abs().max()) == 0.0, "the idle deterministic actor of the critic's object is never touched"


def test_graph_replay_equals_eager_bit_for_bit_under_injected_noise_and_follows_the_learning_rate():
    """Three process() calls of three learns each, cosine decay over 40 steps: the first learn runs eagerly, the second is captured, seven are
    replayed -- the same bits as an agent that never captures: weights, targets, moments, multipliers, results."""
    agents = [_small_agent(use_graph=g) for g in (True, False)]
    assert torch.equal(_state(agents[0]), _state(agents[1])), "one torch.manual_seed, the same initial weights"
    for call in range(3):
        res = []
        for a in agents:
            np.random.seed(7 + call)
            a._noise_inject = _eps(a, call)
            res.append(a.process(_rows(call), 10 * (call + 1)))
        torch.cuda.synchronize()
        assert res[0] == res[1] and set(res[0]) == set(D.STATS), call
        assert torch.equal(_state(agents[0]), _state(agents[1])), call
    assert agents[0].num_learn == 9 and agents[0]._lr_now == pytest.approx(1e-3 * np.cos(0.5 * np.pi * 30 / 40))
    assert torch.equal(agents[0]._actor.target, agents[0]._actor.params) and torch.equal(agents[0]._critic.target, agents[0]._critic.params)
    # without injection the normals are fresh draws in front of every replay: two learns on the same rows differ
    a = agents[0]
    a._noise_inject = None
    np.random.seed(1)
    r1 = a.learn()
    z1 = a._static["z"].clone()
    np.random.seed(1)
    r2 = a.learn()
    torch.cuda.synchronize()
    assert not torch.equal(z1, a._static["z"]) and r1["actor_loss"] != r2["actor_loss"]


def test_save_load_roundtrip_in_the_reference_format_and_full_resume(tmp_path):
    from jorldy_amd.core.network import Network

    agent = _small_agent()
    for call in range(2):
        np.random.seed(call)
        agent._noise_inject = _eps(agent, call)
        agent.process(_rows(call), 10 * (call + 1))
    agent.save(str(tmp_path))
    ck = torch.load(str(tmp_path / "ckpt"), map_location="cpu", weights_only=False)
    assert set(ck) == {"actor", "critic", "actor_optimizer", "critic_optimizer"}
    actor, critic = Network("continuous_policy", 4, 3, D_hidden=32, head="mlp"), Network("continuous_q_network", 4, 3, D_hidden=32, head="mlp")
    actor.load_state_dict(ck["actor"])
    critic.load_state_dict(ck["critic"])
    scalars = [torch.nn.Parameter(torch.tensor(1.0)) for _ in range(3)]
    opt_a, opt_c = torch.optim.Adam(list(actor.parameters()) + scalars, lr=1e-3), torch.optim.Adam(critic.parameters(), lr=1e-3)
    opt_a.load_state_dict(ck["actor_optimizer"])
    opt_c.load_state_dict(ck["critic_optimizer"])
    blk = agent.multipliers()
    for j, n in enumerate(D.NAMES):  # all three multipliers have optimizer state, alpha_sigma's entry included
        assert float(opt_a.state[scalars[j]]["exp_avg"]) == np.float32(blk[n]["m"]) and float(opt_a.state[scalars[j]]["exp_avg_sq"]) == np.float32(blk[n]["v"]), n
    assert float(opt_a.state[scalars[2]]["step"]) == 6.0 == float(opt_c.state[next(iter(critic.parameters()))]["step"])
    other = _small_agent()
    other.load(str(tmp_path))
    torch.cuda.synchronize()
    for a, b in ((agent._actor, other._actor), (agent._critic, other._critic)):
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(b.target, b.params)
    mo = other.multipliers()
    for n in D.NAMES:
        assert (mo[n]["m"], mo[n]["v"], mo[n]["has_state"]) == (blk[n]["m"], blk[n]["v"], True)
    assert other._adam_steps == 6 and other._lr_now == pytest.approx(agent._lr_now)
    # the complete checkpoint: a resumed run continues bit for bit
    full = tmp_path / "full"
    full.mkdir()
    agent.save_full(str(full))
    resumed = _small_agent(eta=1.0, alpha_mu=1.0)
    resumed.load_full(str(full))
    torch.cuda.synchronize()
    assert torch.equal(_state(agent), _state(resumed)) and resumed.memory.size == agent.memory.size == 16
    out = []
    for a in (agent, resumed):
        np.random.seed(11)
        a._noise_inject = _eps(a, 5)
        out.append(a.process(_rows(2), 30))
    torch.cuda.synchronize()
    assert out[0] == out[1] and torch.equal(_state(agent), _state(resumed))
    # sync carries the actor only
    payload = agent.sync_out()
    fresh = _small_agent(seed=6)
    before = fresh._critic.params.clone()
    fresh.sync_in(payload["weights"])
    assert list(payload["weights"])[-1] == "log_std.bias" and torch.equal(fresh._actor.params, agent._actor.params) and torch.equal(fresh._critic.params, before)


@pytest.mark.parametrize("rows", [1, 5])
def test_act_shapes_and_prob(rows):
    agent = _small_agent()
    with torch.no_grad():
        agent._actor.params.add_(0.3 * torch.randn_like(agent._actor.params))
    x = np.random.RandomState(rows).randn(rows, 4).astype(np.float32)
    raw32 = agent.actor(agent.as_tensor(x))
    raw = raw32.double().cpu().numpy()
    mu, th = np.clip(raw[:, :3], -5, 5), np.tanh(raw[:, 3:])
    for training in (True, False):
        torch.manual_seed(1)
        out = agent.act(x, training)
        assert set(out) == {"action", "prob"} and out["action"].shape == (rows, 3) and out["prob"].shape == (rows, 1) and out["action"].dtype == np.float32
        assert np.abs(out["action"]).max() <= 1.0
        if training:  # the same generator state draws the same z: Normal(mu, std).sample() as act() evaluates it
            torch.manual_seed(1)
            z = torch.distributions.Normal(torch.clamp(raw32[:, :3], -5.0, 5.0), torch.tanh(raw32[:, 3:]).exp()).sample()
            assert np.array_equal(out["action"], torch.tanh(z).cpu().numpy()), "the action is tanh of the draw"
            z = z.double().cpu().numpy()
        else:
            z = mu
            np.testing.assert_allclose(out["action"], np.tanh(mu), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(out["prob"][:, 0], np.exp(D.log_prob(z, mu, th)), rtol=1e-5, err_msg="prob = exp(sum_A log N(z; mu, std)) of the z behind the action")


CONFIGS = [("pendulum", dict(state_size=3, action_size=1, batch_size=64, n_step=4, n_epoch=4, critic_loss_type="retrace")),
           ("hopper_mlagent", dict(state_size=76, action_size=3, batch_size=32, n_step=1, n_epoch=4, critic_loss_type="1step_TD"))]


@pytest.mark.parametrize("label,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_reference_config_shapes_construct_and_learn(label, kw):
    """The continuous configurations under config/mpo/ at their shapes (H 512, N 30; n_epoch cut to 4): construction, one process(), finite
    results, moved weights, targets equal to their online nets, all three multipliers stepped."""
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    agent = Agent("mpo", device="cuda", actor="continuous_policy", critic="continuous_q_network", start_train_step=0, run_step=100000, **kw)
    agent.memory.first_store = False
    w0 = _state(agent)
    np.random.seed(0)
    result = agent.process(D.replay(3, kw["batch_size"], agent.n_step, kw["state_size"], kw["action_size"], done_rows=(0, 5)), 1)
    torch.cuda.synchronize()
    assert tuple(result) == D.STATS and all(np.isfinite(v) for v in result.values()), result
    assert agent.num_learn == 4 and not torch.equal(w0, _state(agent))
    assert torch.equal(agent._actor.target, agent._actor.params) and torch.equal(agent._critic.target, agent._critic.params)
    assert result["alpha_sigma"] != 1.0 and result["eta"] != 1.0 and result["alpha_mu"] != 1.0


# ---------------------------------------------------------------------------------------------- the agent against the reference's fixtures
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


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name):
    """Every learn of the fixture on ONE agent with the recorded numpy seed and the recorded normals injected (eps = (z - mu) / std of the
    reference's own draws): the same sampled rows; the raw head of online(s) and mu / std of the other two policies, the four critic outputs
    (rtol and atol 1e-5, tests/test_mpo_gpu.py's for network outputs); z against the tapped z; every result key; head gradients and dQ; where sums
    over the samples enter (actor_loss, eta_loss, alpha_loss, the head gradient) the bound is 2 x the reference's own float32 error + 1e-5, stored
    in the fixture; the multipliers after their step and their moments; both nets' clipped parameter gradients and end weights by the rules of
    tests/test_mpo_gpu.py.  Then a second agent runs the same through process(): the same bits, and targets equal to their online nets."""
    fx = D.Fixture(name)
    agent = _agent_for(fx)
    rows = fx.replay()
    agent.memory.store(rows)
    np.random.seed(fx.np_seed)
    R, A, NS = fx.R, fx.A, fx.NS
    result, injected = None, []
    for k in range(fx.learns):
        rec = fx.learn(k)
        injected.append(rec["eps"])
        agent._noise_inject = rec["eps"]
        mult_before = agent.multipliers()
        result = agent.learn()
        torch.cuda.synchronize()
        st = agent._static
        assert tuple(result) == D.STATS and np.array_equal(npy(st["idx"]), rec["idx"]), "other rows were sampled"
        if k == 0:
            assert [mult_before[n]["value"] for n in D.NAMES] == [float(rec[f"mult0/{n}"]) for n in D.NAMES]
        la = npy(st["la"]).reshape(3, R, 2 * A).astype(np.float64)
        pol = lambda h: (np.clip(h[:, :A], -5, 5), np.exp(np.tanh(h[:, A:])))
        close = lambda ours, key: np.testing.assert_allclose(fx.thin(ours), rec[key].reshape(np.shape(fx.thin(ours))), rtol=1e-5, atol=1e-5, err_msg=f"l{k} {key}")
        close(la[0], "head")
        for (m, s), (km, ks) in ((pol(la[0]), ("mu", "std")), (pol(la[1]), ("next_mu", "next_std")), (pol(la[2]), ("mut", "stdt"))):
            close(m, km)
            close(s, ks)
        for ours, key in ((st["z"][0], "zn"), (st["z"][1], "zt_add")):
            np.testing.assert_allclose(fx.thin(npy(ours)), rec[key].reshape(np.shape(fx.thin(npy(ours)))), rtol=1e-5, atol=2e-5, err_msg=f"l{k} {key} against the tapped z")
        for ours, key in zip(st["lq"], ("q", "qt_a", "qt_next", "qt_add")):
            close(npy(ours), key)
        for key in D.STATS:
            print(f"{name} l{k} {key}: ours {result[key]!r} reference {float(rec['result/' + key])!r}")
        for key in ("actor_loss", "eta_loss", "alpha_loss"):
            np.testing.assert_allclose(result[key], float(rec[f"result/{key}"]), rtol=fx.tol(key), err_msg=f"l{k} {key}")
        for key in ("critic_loss", "min_Q", "max_Q"):
            np.testing.assert_allclose(result[key], float(rec[f"result/{key}"]), rtol=1e-5, err_msg=f"l{k} {key}")
        for key in ("min_At", "max_At"):
            np.testing.assert_allclose(result[key], float(rec[f"result/{key}"]), rtol=fx.tol("At"), atol=1e-6, err_msg=f"l{k} {key}")
        for ours, key, tol in ((st["g_la"], "d_head", fx.tol("d_head")), (st["g_q"], "d_q", 1e-5)):
            ref = rec[key]
            margins.leq(float(np.abs(fx.thin(npy(ours)) - ref.reshape(np.shape(fx.thin(npy(ours))))).max()) / float(np.abs(ref).max()), tol, f"l{k} {key}: max |diff| / the tensor's largest entry")
        blk = agent.multipliers()
        for j, n in enumerate(D.NAMES):
            x0, w = float(rec[f"mult0/{n}"]), float(rec[f"mult1/{n}"])
            margins.leq(abs(result[n] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * fx.lr, f"l{k} {n} after its step")
            assert blk[n]["value"] == result[n] and blk[n]["has_state"]
            np.testing.assert_allclose(blk[n]["m"], float(rec[f"mult1/{n}/exp_avg"]), rtol=2e-5, atol=1e-9, err_msg=f"l{k} {n} exp_avg")
            np.testing.assert_allclose(blk[n]["v"], float(rec[f"mult1/{n}/exp_avg_sq"]), rtol=2e-5, err_msg=f"l{k} {n} exp_avg_sq")
        assert agent._adam_steps == k + 1
        for label, net, view in (("actor", agent._actor, agent.actor), ("critic", agent._critic, agent.critic)):
            for key, g in net.export_state(net.grads).items():  # the bucket holds the clipped gradient after the optimizer step
                ref = rec[f"grad_clip/{label}/{key}"]
                coef = min(1.0, fx.clip / (float(rec[f"grad_raw_norm/{label}"]) + 1e-6))
                scale = float(rec[f"grad_raw_absmax/{label}/{key}"]) * coef
                margins.leq(float(np.abs(fx.thin(npy(g)) - ref.reshape(np.shape(fx.thin(npy(g))))).max()) / scale, fx.tol("d_head") if label == "actor" else 1e-5,
                            f"l{k} clipped d(loss)/d {label}.{key}: max |diff| / the tensor's largest entry")
            tot = bad = 0
            worst = 0.0
            for key, v in view.state_dict().items():
                dd = np.abs(fx.thin(npy(v)) - rec[f"sd1/{label}/{key}"].reshape(np.shape(fx.thin(npy(v)))))
                tot += dd.size
                bad += int((dd > 2e-5).sum())
                worst = max(worst, float(dd.max()) / fx.lr)
            margins.leq(bad / tot, 0.005, f"l{k} {label}: fraction of weights further than 2e-5 from the reference's")
            margins.leq(worst, 2.1, f"l{k} {label}: worst weight difference / lr vs the possible travel")
    if name == "mpo_cont_td":
        assert result["alpha_sigma"] == float(np.float32(fx.floors[2])), "the first step of alpha_sigma is clamped to its floor"
    # the same through process(): store, `learns` learns, hard target update
    other = _agent_for(fx)
    np.random.seed(fx.np_seed)
    draws = iter(injected)
    draw = type(other)._draw

    def _draw(st):  # learn k of process() takes the normals of learn k
        other._noise_inject = next(draws)
        draw(other, st)

    other._draw = _draw
    res2 = other.process(rows, 1)
    torch.cuda.synchronize()
    assert res2 == result
    for a, b in ((agent._actor, other._actor), (agent._critic, other._critic)):
        assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
        assert torch.equal(b.target, b.params) and not torch.equal(a.target, a.params), "process() ends with the hard copies of both nets"
    assert torch.equal(agent._mult, other._mult)
