"""SAC on the GPU: the kernels of jh_sac.hip (sample, critic loss, actor seed with the temperature's bookkeeping, sample backward) and the
network object (ops.SACNet) against the float64 truth of tests/sac_truth.py (pinned to the reference's own learn() and to the case builders'
conditions by tests/test_sac_cpu.py) and against the fixtures of tools/gen_golden_sac.py; then the whole agent: one learn() per fixture record
with both normal draws injected (the second of two consecutive learns pins the one-step lag of alpha), hipGraph replay against eager,
acting on torch's own generator, the configs' shapes, checkpoints, and the learning curve on the control env next to the reference's."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import sac_truth as D
from tests.util import f32, load, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5


# ----------------------------------------------------------------------------------------------- sample forward
@pytest.mark.parametrize("s", D.SPREADS)
@pytest.mark.parametrize("B,A", D.SAMPLE_SHAPES)
def test_sample_matches_float64(B, A, s):
    """a within 4 * 2^-24; logp per row within K = 4 times the float32 rounding bound of sac_truth.logp_bound (the reference's own float32
    evaluation needs K <= 1 on these inputs: test_sac_cpu)."""
    from jorldy_amd import ops

    mu, ls, eps = D.sample_case(B, A, s)
    a, logp = ops.sac_sample(f32(mu), f32(ls), f32(eps))
    a64, lp64 = D.sample(mu, ls, eps)
    ea = float(np.abs(npy(a).astype(np.float64) - a64.numpy()).max())
    margins.leq(ea, 4 * 2.0 ** -24, f"B{B} A{A} s{s} |a - fp64|")
    assert float(np.abs(npy(a)).max()) <= 1.0
    err = np.abs(npy(logp).astype(np.float64) - lp64.numpy())
    bound = D.logp_bound(eps, a64.numpy(), 4.0)
    i = int(np.argmax(err / bound))
    print(f"B{B} A{A} s{s}: |a - fp64| = {ea / 2.0 ** -24:.2f} x 2^-24, logp needs K = {4 * float(err[i] / bound[i]):.3f}")
    margins.leq(float(err[i]), float(bound[i]), f"B{B} A{A} s{s} |logp - fp64| row {i} against K = 4")
    # evaluation: tanh(clamp(mu_raw)), no logp
    ev, none = ops.sac_sample(f32(mu))
    assert none is None
    margins.leq(float(np.abs(npy(ev).astype(np.float64) - np.tanh(np.clip(mu.astype(np.float64), -5, 5))).max()), 4 * 2.0 ** -24, "evaluation action")


def test_sample_is_bit_identical_across_runs_and_rejects_bad_sizes():
    from jorldy_amd import _lib, ops

    mu, ls, eps = (f32(x) for x in D.sample_case(257, 2, 1.5))
    a1, l1 = ops.sac_sample(mu, ls, eps)
    a2, l2 = ops.sac_sample(mu, ls, eps)
    assert torch.equal(a1, a2) and torch.equal(l1, l2)
    z = torch.zeros(0, 3, device="cuda")
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.sac_sample(z, z, z)
    z = torch.zeros(3, 0, device="cuda")
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.sac_sample(z, z, z)


# ----------------------------------------------------------------------------------------------- sample backward
@pytest.mark.parametrize("s", D.SPREADS)
@pytest.mark.parametrize("B,A", D.SAMPLE_SHAPES)
def test_sample_backward_matches_float64_autograd(B, A, s):
    """Elements with 1 - a^2 >= 1e-3 in the truth: fp64_truth.grad_vs_exact at TOL against float64 autograd, torch-CPU-float32 autograd
    beside it.  The rest is ill conditioned in the reference itself (float32 1 - a^2 is 0 where float64 is not): finite, and
    |dz| <= |da| + 2 alpha / B."""
    from jorldy_amd import ops

    mu, ls, eps = D.sample_case(B, A, s)
    da = D.sample_da(B, A)
    blk = ops.sac_alpha_block(0.0, alpha=D.ALPHA, dynamic=False, target_entropy=-A)
    blk[9] = float(np.float32(D.ALPHA) / np.float32(B))
    a, _ = ops.sac_sample(f32(mu), f32(ls), f32(eps))
    dmu, dls = ops.sac_sample_backward(f32(da), f32(mu), f32(ls), f32(eps), a, blk)
    # the two critics' halves summed by the kernel
    dmu2, dls2 = ops.sac_sample_backward(f32(da * 0.25), f32(mu), f32(ls), f32(eps), a, blk, grad_a2=f32(da * 0.75))
    assert torch.equal(dmu, dmu2) and torch.equal(dls, dls2)  # 0.25 x + 0.75 x is x exactly in binary floating point
    g64 = D.sample_backward(da, mu, ls, eps, D.ALPHA)
    g32 = D.sample_backward(da, mu, ls, eps, D.ALPHA, torch.float32)
    well = (1 - g64[2].numpy() ** 2) >= D.WELL
    assert 1 - well.mean() <= 0.30
    dmu, dls = npy(dmu), npy(dls)
    e1 = T.grad_vs_exact(dmu, g64[0].numpy(), g32[0].numpy(), TOL, f"B{B} A{A} s{s} d(mu_raw)", rows=well)
    e2 = T.grad_vs_exact(dls, g64[1].numpy(), g32[1].numpy(), TOL, f"B{B} A{A} s{s} d(ls_raw)", rows=well)
    print(f"B{B} A{A} s{s}: d(mu_raw) {e1[0]:.2e} (fp32 {e1[1]:.2e}), d(ls_raw) {e2[0]:.2e} (fp32 {e2[1]:.2e}), {100 * (1 - well.mean()):.1f} % left out")
    assert np.isfinite(dmu).all() and np.isfinite(dls).all()
    inside = np.abs(mu) <= 5
    lim = np.abs(da.astype(np.float64)) + 2 * D.ALPHA / B
    assert np.all(np.abs(dmu.astype(np.float64))[inside] <= lim[inside]), "|dz| <= |da| + 2 alpha / B"
    # the clamp: element 0 is outside (exactly 0), element 1 sits on the bound (the gradient passes)
    assert dmu.reshape(-1)[0] == 0.0 and np.all(dmu[np.abs(mu) > 5] == 0.0)
    if B * A > 1:
        assert dmu.reshape(-1)[1] != 0.0


# ----------------------------------------------------------------------------------------------- critic loss and actor seed
@pytest.mark.parametrize("variant", D.LOSS_VARIANTS)
@pytest.mark.parametrize("B", D.LOSS_B)
def test_critic_loss_and_actor_seed_match_float64(B, variant):
    """y, both losses, max_Q, dq and the seed's statistics against float64 at the tolerances of test_td3_gpu's
    test_critic_loss_matches_float64_truth: gradients by grad_vs_exact at TOL, every scalar at rtol 1e-5 with no absolute term."""
    from jorldy_amd import ops

    q, qn, lp, lpn, r, d = D.loss_case(B, variant)
    gamma, alpha, la = 0.99, 0.37, -0.8
    blk = ops.sac_alpha_block(la, alpha=alpha, dynamic=False, target_entropy=-3.0)
    y, grad, st = ops.sac_critic_loss(f32(q), f32(qn), f32(lpn), f32(r), f32(d), gamma, blk, stats=torch.full((4,), -1.0, device="cuda"))
    a32 = float(np.float32(alpha))
    t, t32 = D.critic_loss(q, qn, lpn, r, d, gamma, a32), D.critic_loss(q, qn, lpn, r, d, gamma, a32, torch.float32)
    T.grad_vs_exact(npy(y), t["y"].numpy(), t32["y"].numpy(), TOL, "y")
    e = T.grad_vs_exact(npy(grad), t["grad"].numpy(), t32["grad"].numpy(), TOL, "d(loss_i)/d(q_i)")
    st = npy(st)
    assert st[3] == 0.0, "arrival mark"
    for i in range(2):
        np.testing.assert_allclose(st[i], float(t["loss"][i]), rtol=1e-5, err_msg=f"loss_{i + 1}")
    np.testing.assert_allclose(st[2], float(t["max_Q"]), rtol=1e-5, err_msg="max_Q")
    if variant == "all_done":
        np.testing.assert_array_equal(npy(y), r)
    # ---- the actor seed (static temperature: the block but for the coefficient is only read)
    before = blk.clone()
    dq, st = ops.sac_actor_seed(f32(q), f32(lp), blk, stats=torch.full((6,), -1.0, device="cuda"))
    la32 = float(np.float32(la))
    s, s32 = D.actor_seed(q, lp, a32, la32, -3.0), D.actor_seed(q, lp, a32, la32, -3.0, torch.float32)
    T.grad_vs_exact(npy(dq), s["grad"].numpy(), s32["grad"].numpy(), TOL, "d(actor_loss)/d(q_i)")
    g = np.float32(-1.0) / np.float32(B)
    if variant == "equal_q":
        assert np.array_equal(npy(dq), np.full((2, B), np.float32(0.5) * g, np.float32)), "half each on a tie"
    else:
        assert np.array_equal(npy(dq).sum(0), np.full(B, g, np.float32)) and np.all((npy(dq) == 0).sum(0) == 1)
    st = npy(st)
    assert st[5] == 0.0, "arrival mark"
    for i, k in ((0, "actor_loss"), (1, "alpha_loss"), (2, "mean_Q"), (4, "entropy")):
        np.testing.assert_allclose(st[i], float(s[k]), rtol=1e-5, err_msg=k)
    assert st[3] == np.float32(alpha), "a static temperature is reported as it stands"
    after = npy(blk)
    assert after[9] == np.float32(alpha) / np.float32(B) and float(s["coef"][0]) == pytest.approx(after[9], rel=1e-6)
    after[9] = npy(before)[9]
    assert np.array_equal(after.view(np.uint32), npy(before).view(np.uint32)), "a static temperature block moved"
    print(f"B{B} {variant}: critic gradient |ours - fp64| / max = {e[0]:.3e}")


def test_losses_are_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B in (256, 1025, 7):
        q, qn, lp, lpn, r, d = (f32(a) for a in D.loss_case(B, "plain", seed=1))
        mk = lambda: ops.sac_alpha_block(0.0, lr=5e-2, dynamic=True, target_entropy=-2.0)
        b1, b2, b3 = mk(), mk(), mk()
        run = lambda blk: ops.sac_critic_loss(q, qn, lpn, r, d, 0.99, blk) + ops.sac_actor_seed(q, lp, blk)
        o1, o2 = run(b1), run(b2)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(o1, o2)) and torch.equal(b1, b2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            o3 = run(b3)
        b3.copy_(mk())
        for t in o3:
            t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(o1, o3)) and torch.equal(b1, b3)
        # a second replay is a second learn: it sees the alpha the first one refreshed and takes Adam's second step
        run(b1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(b1, b3) and ops.sac_alpha_read(b3)["step"] == 2


def test_losses_reject_out_of_range_sizes():
    from jorldy_amd import _lib, ops

    blk = ops.sac_alpha_block(0.0)
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.sac_critic_loss(z(2, 0), z(2, 0), z(0), z(0), z(0), 0.99, blk)
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.sac_actor_seed(z(2, 0), z(0), blk)
    n = (1 << 20) + 1
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.sac_critic_loss(z(2, n), z(2, n), z(n), z(n), z(n), 0.99, blk)
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.sac_actor_seed(z(2, n), z(n), blk)


# ----------------------------------------------------------------------------------------------- the temperature
def test_alpha_step_static_stays_and_dynamic_lags_by_one_step():
    from jorldy_amd import ops

    B, lr, te = 257, 5e-2, -3.0
    q = f32(np.zeros((2, B), np.float32))
    # static: three seeds, nothing moves
    blk = ops.sac_alpha_block(-2.0, dynamic=False, target_entropy=te)
    start = ops.sac_alpha_read(blk)
    assert start["alpha"] == float(np.float32(np.exp(np.float64(np.float32(-2.0)))))
    for k in range(3):
        _, st = ops.sac_actor_seed(q, f32(D.loss_case(B, "plain", seed=k)[2]), blk)
        now = ops.sac_alpha_read(blk)
        assert {k_: v for k_, v in now.items() if k_ != "coef"} == {k_: v for k_, v in start.items() if k_ != "coef"}
        assert float(st[3]) == start["alpha"]
    # dynamic: three consecutive steps, each against float64 Adam started from OUR state before the step
    blk = ops.sac_alpha_block(0.0, lr=lr, dynamic=True, target_entropy=te)
    used = []
    for k in range(3):
        lp = D.loss_case(B, "plain", seed=k)[2]
        before = ops.sac_alpha_read(blk)
        _, st = ops.sac_actor_seed(q, f32(lp), blk)
        after = ops.sac_alpha_read(blk)
        used.append(before["alpha"])
        # the loss of this step was formed with the alpha in use BEFORE it; the block now holds exp(log_alpha before the Adam step)
        assert after["coef"] == float(np.float32(before["alpha"]) / np.float32(B))
        np.testing.assert_allclose(after["alpha"], np.exp(before["log_alpha"]), rtol=4e-7, err_msg="alpha in use = exp(log_alpha) of before the step")
        assert float(st[3]) == after["alpha"] and after["step"] == k + 1
        g = float(D.actor_seed(npy(q), lp, before["alpha"], before["log_alpha"], te)["alpha_grad"])
        w, m, v = D.alpha_adam_step(before["log_alpha"], g, before["m"], before["v"], before["step"], lr)
        allowed = 2.0 ** -22 * abs(w) + 1e-4 * abs(w - before["log_alpha"]) + 1e-6 * lr
        margins.leq(abs(after["log_alpha"] - w), allowed, f"log_alpha after step {k + 1} vs float64 Adam")
        margins.leq(abs(after["m"] - m), 1e-5 * abs(m), f"exp_avg after step {k + 1}")
        margins.leq(abs(after["v"] - v), 1e-5 * abs(v), f"exp_avg_sq after step {k + 1}")
        np.testing.assert_allclose(float(st[1]), before["log_alpha"] * g, rtol=1e-5, err_msg="alpha_loss")
    # learns 0 and 1 both use the initial alpha; learn 2 uses exp(log_alpha after ONE step)
    assert used[0] == 1.0 and used[1] == 1.0 and used[2] != 1.0
    first = D.alpha_adam_step(0.0, float(D.actor_seed(npy(q), D.loss_case(B, "plain", seed=0)[2], 1.0, 0.0, te)["alpha_grad"]), 0, 0, 0, lr)[0]
    np.testing.assert_allclose(used[2], np.exp(first), rtol=1e-5, err_msg="the alpha of learn 2 is exp(log_alpha) after one step")


# ----------------------------------------------------------------------------------------------- the network object
class Twin(torch.nn.Module):
    """The online critics as ONE module, so that fp64_truth.OptimTruth steps them with one torch.optim.Adam as the native object does."""

    def __init__(self, critics):
        super().__init__()
        self.c = torch.nn.ModuleList(critics)


def _twin_state(nat, kind):
    out = OrderedDict()
    for c in range(2):
        for k, v in nat.export_state(f"critic{c + 1}", kind).items():
            out[f"c.{c}.{k}"] = v
    return out


def _force(nat, truth, which, lr, it):
    """Teacher-force the native object: parameters and moments of the float64 trajectory, rounded to float32."""
    params, m, v = truth.teacher_force()
    nets = ("actor",) if which == "actor" else ("critic1", "critic2")
    for c, net in enumerate(nets):
        pick = (lambda d: d) if which == "actor" else (lambda d: {k[len(f"c.{c}."):]: t for k, t in d.items() if k.startswith(f"c.{c}.")})
        nat.import_state(pick(params), net)
        for kind, src in (("m", m), ("v", v)):
            if src is not None:
                nat.import_state(pick(src), net, kind)
            else:
                nat.flat(net, kind).zero_()
    nat.set_hyper(which, lr, 0.9, 0.999, 1e-8, it)


@pytest.mark.parametrize("S,A,H,B", D.NET_SHAPES)
def test_sacnet_forwards_critic_update_and_actor_update_match_float64(S, A, H, B):
    from jorldy_amd import ops

    steps = 3
    a64, a32 = D.mirrors(D.Actor, S, A, H, 0)
    cs = [D.mirrors(D.Critic, S, A, H, 1 + c) for c in range(2)]
    tcs = [D.mirrors(D.Critic, S, A, H, 101 + c) for c in range(2)]
    tw64, tw32 = Twin([c[0] for c in cs]), Twin([c[1] for c in cs])
    nat = ops.SACNet(S, A, H, B, "cuda:0")
    assert nat.nets() == ("actor", "critic1", "critic2")
    nat.import_state(a32.state_dict(), "actor")
    for c in range(2):
        nat.import_state(cs[c][1].state_dict(), f"critic{c + 1}")
        nat.import_state(tcs[c][1].state_dict(), f"critic{c + 1}", "target")
    nat.set_alpha(-1.5, dynamic=False)
    blk = nat.get_alpha()
    alpha, log_alpha, te = blk["alpha"], blk["log_alpha"], blk["target_entropy"]
    assert te == -A and not blk["dynamic"] and alpha == float(np.float32(np.exp(-1.5)))
    # ---- export / import round trip under the reference's keys
    sd = nat.export_state("actor")
    assert tuple(sd.keys()) == D.ACTOR_KEYS == tuple(a32.state_dict().keys())
    for k, v in a32.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k
    for c in range(2):
        for kind, src in (("params", cs[c][1]), ("target", tcs[c][1])):
            sd = nat.export_state(f"critic{c + 1}", kind)
            assert tuple(sd.keys()) == D.CRITIC_KEYS
            for k, v in src.state_dict().items():
                assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), (c, kind, k)
    with pytest.raises(KeyError):
        nat.import_state({"head.l.weight": torch.zeros(H, S)}, "actor")
    with pytest.raises(KeyError):
        nat.flat("actor", "target")  # the actor is online only
    # ---- both forwards
    x, act, critic_in, actor_in = D.net_inputs(S, A, B, steps)
    with torch.no_grad():
        mu, std = nat.actor_forward(x.cuda())
        for got, i, what in ((mu, 0, "mu"), (std, 1, "std")):
            T.vs_exact(got, a64(x.double())[i], a32(x)[i], TOL, f"actor forward {what}")
        for which, nets in enumerate((cs, tcs)):
            q = nat.critic_forward(x.cuda(), act.cuda(), which)
            for c in range(2):
                T.vs_exact(q[c], nets[c][0](x.double(), act.double()), nets[c][1](x, act), TOL, f"critic{c + 1} forward which={which}")
        if B > 1:
            T.vs_exact(nat.actor_forward(x[:1].cuda().contiguous())[0], a64(x[:1].double())[0], a32(x[:1])[0], TOL, "actor forward, one row")
    # ---- the critic update: the online actor on s', target pass, online pass, loss, backward, three teacher-forced Adam steps
    lr, gamma = 1e-3, 0.99
    actor_before = {kind: nat.actor[kind].clone() for kind in nat.AKINDS}
    truth = T.OptimTruth(tw64, tw32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    for it, ci in enumerate(critic_in):
        _force(nat, truth, "critic", lr, it)
        xa, act, r, d, eps = (ci[k] for k in ("x_all", "action", "reward", "done", "eps"))
        dev = lambda *shape: torch.empty(*shape, device="cuda")
        stats, y, q, a2, lp2 = torch.full((4,), -1.0, device="cuda"), dev(B), dev(2, B), dev(B, A), dev(B)
        nat.critic_update(xa.cuda(), act.cuda(), r.cuda(), d.cuda(), eps.cuda(), gamma, stats, y=y, q=q, a_next=a2, logp_next=lp2)
        ref = {}
        for dt, tw, actor, tcs_ in ((torch.float64, tw64, a64, [t[0] for t in tcs]), (torch.float32, tw32, a32, [t[1] for t in tcs])):
            c = lambda t: t.to(dt)
            with torch.no_grad():
                an, lpn = D.sample(*actor.raw(c(xa[B:])), eps, dt)
                nq = torch.min(tcs_[0](c(xa[B:]), an), tcs_[1](c(xa[B:]), an))
                yy = c(r).view(-1, 1) + (1 - c(d).view(-1, 1)) * gamma * (nq + alpha * (-lpn.view(-1, 1)))
            for p in tw.parameters():
                p.grad = None
            qs = [crit(c(xa[:B]), c(act)) for crit in tw.c]
            losses = [torch.nn.functional.mse_loss(qq, yy) for qq in qs]
            sum(losses).backward()
            ref[dt] = (yy, qs, losses, an, lpn)
        (y64, q64, l64, an64, lp64), (y32, q32, l32, an32, lp32) = ref[torch.float64], ref[torch.float32]
        T.vs_exact(a2, an64, an32, TOL, f"step {it} a'")
        T.vs_exact(lp2, lp64, lp32, TOL, f"step {it} logp'")
        T.vs_exact(y, y64, y32, TOL, f"step {it} y")
        st = npy(stats)
        assert st[3] == 0.0
        for c in range(2):
            T.vs_exact(q[c], q64[c].detach(), q32[c].detach(), TOL, f"step {it} q{c + 1}")
            T.vs_exact(torch.tensor(st[c]), l64[c].detach(), l32[c].detach(), TOL, f"step {it} critic_loss{c + 1}")
        T.vs_exact(torch.tensor(st[2]), y64.max(), y32.max(), TOL, f"step {it} max_Q")
        raw = _twin_state(nat, "grads")
        p32 = dict(tw32.named_parameters())
        for k, p in tw64.named_parameters():
            T.vs_exact(raw[k], p.grad, p32[k].grad, TOL, f"step {it} grad {k}")
        truth.step(None, raw, _twin_state(nat, "params"), _twin_state(nat, "m"), _twin_state(nat, "v"), tag=f"critic adam step {it}")
    for kind in nat.AKINDS:
        assert torch.equal(nat.actor[kind], actor_before[kind]), f"the critic update wrote the actor's {kind} bucket"
    # ---- the actor update: through both critics' action inputs and through logp, the actor's Adam; the critics are not written
    atruth = T.OptimTruth(a64, a32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    for it, ai in enumerate(actor_in):
        _force(nat, atruth, "actor", lr, it)
        xs, eps = ai["x"], ai["eps"]
        before = {kind: nat.critics[kind].clone() for kind in nat.KINDS}
        dev = lambda *shape: torch.empty(*shape, device="cuda")
        stats, a_pred, lp, qpi = torch.full((6,), -1.0, device="cuda"), dev(B, A), dev(B), dev(2, B)
        nat.actor_update(xs.cuda(), eps.cuda(), stats, action=a_pred, logp=lp, q=qpi)
        torch.cuda.synchronize()
        for kind in nat.KINDS:
            assert torch.equal(nat.critics[kind], before[kind]), f"the actor update wrote the critics' {kind} bucket"
        sds = [{k: v.cpu() for k, v in nat.export_state(f"critic{c + 1}").items()} for c in range(2)]
        ref = {dt: D.actor_update(None, None, xs, eps, alpha, log_alpha, te, dt, actor=actor, critics=[D.build(D.Critic, sd_, dt) for sd_ in sds])
               for dt, actor in ((torch.float64, a64), (torch.float32, a32))}
        r64, r32 = ref[torch.float64], ref[torch.float32]
        assert float(torch.atanh(r64["action"].abs().clamp(max=1 - 1e-12)).max()) <= 4.0, "the case builder keeps max |z| <= 4"
        T.vs_exact(a_pred, r64["action"], r32["action"], TOL, f"actor step {it} a")
        T.vs_exact(lp, r64["logp"], r32["logp"], TOL, f"actor step {it} logp")
        T.vs_exact(torch.min(qpi[0], qpi[1]), r64["min_q"], r32["min_q"], TOL, f"actor step {it} min_q")
        st = npy(stats)
        assert st[5] == 0.0 and st[3] == np.float32(alpha)
        for i, k in ((0, "actor_loss"), (1, "alpha_loss"), (2, "mean_Q"), (4, "entropy")):
            T.vs_exact(torch.tensor(st[i]), r64[k], r32[k], TOL, f"actor step {it} {k}")
        raw = nat.export_state("actor", "grads")
        p32 = dict(a32.named_parameters())
        assert len(raw) == 8
        for k, p in a64.named_parameters():
            T.vs_exact(raw[k], p.grad, p32[k].grad, TOL, f"actor step {it} grad {k}")
        atruth.step(None, raw, nat.export_state("actor"), nat.export_state("actor", "m"), nat.export_state("actor", "v"), tag=f"actor adam step {it}")
    # ---- soft update (the critics' targets only, bit-identical to torch float32 on the CPU) and target sync
    tau = 5e-3
    nets = ("critic1", "critic2")
    want = {net: {k: D.polyak(nat.export_state(net)[k].cpu(), nat.export_state(net, "target")[k].cpu(), tau) for k in nat.export_state(net)} for net in nets}
    actor_before = {kind: nat.actor[kind].clone() for kind in nat.AKINDS}
    nat.soft_update(tau)
    for net in nets:
        for k, v in nat.export_state(net, "target").items():
            assert torch.equal(v.cpu(), want[net][k]), (net, k)
    for kind in nat.AKINDS:
        assert torch.equal(nat.actor[kind], actor_before[kind]), f"the soft update wrote the actor's {kind} bucket"
    nat.sync_target()
    for net in nets:
        assert torch.equal(nat.flat(net, "target"), nat.flat(net))


# ----------------------------------------------------------------------------------------------- the agent
def _agent_for(fx, use_graph=True, **over):
    from jorldy_amd.core.agent import Agent

    z = fx.z
    kw = dict(state_size=fx.S, action_size=fx.A, hidden_size=fx.H, batch_size=fx.B, gamma=float(z["hyper/gamma"]), buffer_size=256, start_train_step=0,
              tau=float(z["hyper/tau"]), run_step=100000, device="cuda", use_graph=use_graph, use_dynamic_alpha=fx.dynamic, static_log_alpha=float(z["hyper/static_log_alpha"]),
              optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": float(z["hyper/actor_lr"]), "critic_lr": float(z["hyper/critic_lr"]),
                            "alpha_lr": float(z["hyper/alpha_lr"])})
    kw.update(over)
    return Agent("sac", **kw)


def _net_of(fx_net):
    """fixture network name -> (ops.SACNet network, bucket)"""
    return fx_net.replace("target_", ""), ("target" if fx_net.startswith("target_") else "params")


def _loaded_agent(fx, **kw):
    agent = _agent_for(fx, **kw)
    for net in fx.nets:
        agent._net.import_state(fx.sd0[net], *_net_of(net))
    agent.memory.first_store = False
    agent.memory.store(fx.buffer())
    return agent


def _cmp(fx, ours, ref, scale, tol, what):
    got = fx.thin(npy(ours) if torch.is_tensor(ours) else ours)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got.astype(np.float64) - ref).max()) / (float(scale) + 1e-30)
    margins.leq(err, tol, f"{what}: max |diff| / the tensor's largest entry")


RESULT_KEYS = {"critic_loss1", "critic_loss2", "actor_loss", "alpha_loss", "max_Q", "mean_Q", "alpha", "entropy"}


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name):
    """One learn() per record from the recorded state with the recorded numpy seed and both normal draws injected: result keys (rtol 1e-5),
    y / q / a / logp (rtol and atol 1e-5), gradients (1e-5 of the tensor's largest entry), Adam moments (2e-5), online weights within the
    caps of test_iqn_agent_learn_matches_reference (at most 0.5 % further than 2e-5 from the reference's, the worst within 2.1 lr); the
    targets are bit-unchanged.  sac.npz: r1 runs as the SECOND learn of the same agent -- weights and moments are set to where the
    reference's r0 ended, the temperature block is left as the device advanced it -- and fails if alpha does not lag by one step."""
    z = load(name)
    fx = D.Fixture(z)
    agent = _loaded_agent(fx)
    net = agent._net
    lrs = {"actor": float(z["hyper/actor_lr"]), "critic": float(z["hyper/critic_lr"])}
    for i, r in enumerate(fx.records):
        if i > 0:  # teacher-force everything but the temperature
            prev = fx.records[i - 1]
            for fnet in fx.nets:
                net.import_state(fx.full(prev, fnet), *_net_of(fnet))
            for onet in net.nets():
                m, v = fx.moments(prev, onet)
                net.import_state(m, onet, "m")
                net.import_state(v, onet, "v")
        al0, al1 = fx.alpha(r, 0), fx.alpha(r, 1)
        blk = net.get_alpha()
        # (float32 exp is correctly rounded neither on the host nor in torch: one unit in the last place)
        np.testing.assert_allclose(blk["alpha"], al0["alpha"], rtol=2e-7, err_msg=f"{r}: the alpha in use")
        assert not fx.dynamic or blk["alpha"] == 1.0, "learns 0 and 1 both use the initial alpha"
        np.testing.assert_allclose(blk["log_alpha"], al0["log_alpha"], rtol=1e-5, err_msg=f"{r} log_alpha before")
        agent._noise_inject = fx.eps(r)
        targets = net.critics["target"].clone()
        np.random.seed(int(z[f"{r}/np_seed"]))
        result = agent.learn()
        torch.cuda.synchronize()
        assert set(result) == RESULT_KEYS and agent.num_learn == i + 1
        for k in sorted(RESULT_KEYS):
            print(f"{name} {r} result {k}: ours {result[k]!r} reference {float(z[f'{r}/result/{k}'])!r}")
            np.testing.assert_allclose(result[k], z[f"{r}/result/{k}"], rtol=1e-5, err_msg=f"{r} {k}")
        assert torch.equal(net.critics["target"], targets), "learn() moved a target"
        st = agent._static
        b = fx.batch(r)
        assert np.array_equal(npy(st["tr"]["state"]), b["state"]) and np.array_equal(npy(st["tr"]["action"]), b["action"].astype(np.float32)), "other rows were sampled"
        flat = lambda k: z[f"{r}/learn/{k}"].reshape(-1)
        for ours, key in ((st["y"], "target_q"), (st["q"][0], "q1"), (st["q"][1], "q2"), (st["a_next"], "next_action"), (st["logp_next"], "next_log_prob"),
                          (st["a_pred"], "sample_action"), (st["logp"], "log_prob"), (st["q_pi"][0], "q1_pi"), (st["q_pi"][1], "q2_pi"),
                          (torch.min(st["q_pi"][0], st["q_pi"][1]), "min_q")):
            np.testing.assert_allclose(npy(ours).reshape(-1), flat(key), rtol=1e-5, atol=1e-5, err_msg=f"{r} {key}")
        tot = bad = 0
        worst = 0.0
        for onet in net.nets():
            for k, v in net.export_state(onet, "grads").items():
                _cmp(fx, v, z[f"{r}/grad/{onet}/{k}"], z[f"{r}/grad_absmax/{onet}/{k}"], 1e-5, f"{r} d(loss)/d {onet} {k}")
            for kind, nm in (("m", "exp_avg"), ("v", "exp_avg_sq")):
                for k, v in net.export_state(onet, kind).items():
                    ref = z[f"{r}/opt/{onet}/{nm}/{k}"]
                    _cmp(fx, v, ref, np.abs(ref).max(), 2e-5, f"{r} {nm} {onet} {k}")
            lr = lrs["actor" if onet == "actor" else "critic"]
            for k, v in net.export_state(onet).items():
                dd = np.abs(fx.thin(npy(v)) - z[f"{r}/sd1/{onet}/{k}"])
                tot += dd.size
                bad += int((dd > 2e-5).sum())
                worst = max(worst, float(dd.max()) / lr)
        margins.leq(bad / tot, 0.005, f"{r} fraction of weights further than 2e-5 from the reference's")
        margins.leq(worst, 2.1, f"{r} worst weight difference / lr vs the possible travel")
        # the temperature after the learn
        blk = net.get_alpha()
        assert blk["alpha"] == result["alpha"] and blk["step"] == al1["step"]
        if fx.dynamic:
            alr = float(z["hyper/alpha_lr"])
            w = al1["log_alpha"]
            margins.leq(abs(blk["log_alpha"] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - al0["log_alpha"]) + 1e-6 * alr, f"{r} log_alpha after its step")
            np.testing.assert_allclose(blk["m"], al1["exp_avg"], rtol=2e-5, err_msg=f"{r} alpha exp_avg")
            np.testing.assert_allclose(blk["v"], al1["exp_avg_sq"], rtol=2e-5, err_msg=f"{r} alpha exp_avg_sq")
        else:
            assert blk["log_alpha"] == al0["log_alpha"] and blk["alpha"] == al0["alpha"] and agent.log_alpha == float(z["hyper/static_log_alpha"])
    assert agent.alpha == net.get_alpha()["alpha"]


def _flat_state(agent):
    n = agent._net
    return torch.cat([n.actor["params"], n.critics["params"], n.critics["target"], n.actor["m"], n.actor["v"], n.critics["m"], n.critics["v"]]).clone()


def test_graph_replay_equals_eager_over_process_calls():
    """Six process() calls with learning-rate decay: the first comes before start_train_step (no learn, no target moves), the other five learn
    -- eager warm-up, capture, three replays -- and each ends with the soft update of the target critics."""
    fx = D.Fixture(load("sac"))
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent = _loaded_agent(fx, use_graph=use_graph, run_step=1000, start_train_step=10)
        np.random.seed(7)
        out, moved, held = [], 0, []
        for it in range(6):
            before = agent._net.critics["target"].clone()
            r = agent.process([fx.buffer()[it]], 5 + 10 * it)
            moved += int(not torch.equal(agent._net.critics["target"], before))
            held.append(sorted(agent._graphs))
            if it == 0:
                assert r == {} and agent.num_learn == 0
            else:
                out.append([r[k] for k in sorted(RESULT_KEYS)])
        assert moved == 5 and agent.num_learn == 5, "the targets have moved five times"
        assert held == ([[], []] + [[(True, True)]] * 4 if use_graph else [[]] * 6), f"captured variants, call by call: {held}"
        assert agent._lr_now["actor"] < agent._lr0["actor"] and agent._net.get_alpha()["lr"] == np.float32(float(fx.z["hyper/alpha_lr"])), "alpha_lr never decays"
        res.append((out, _flat_state(agent), agent._net.get_alpha()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)
    assert res[0][2]["step"] == res[1][2]["step"] == 5
    np.testing.assert_allclose(res[0][2]["log_alpha"], res[1][2]["log_alpha"], rtol=1e-5)


def test_replayed_learns_see_fresh_draws():
    """Learning rates 0, a static alpha and the same sampled rows: consecutive learns differ only in their two normal draws -- and so do the
    critic and actor losses; with the draws injected they give the same bits."""
    fx = D.Fixture(load("sac"))
    torch.manual_seed(0)
    agent = _loaded_agent(fx, lr_decay=False, use_dynamic_alpha=False,
                          optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 0.0, "critic_lr": 0.0, "alpha_lr": 0.0})
    c, a = [], []
    for it in range(6):
        np.random.seed(7)
        r = agent.learn()
        c.append(r["critic_loss1"])
        a.append(r["actor_loss"])
    assert set(agent._graphs) == {(True, False)}
    assert len(set(c)) == 6 and len(set(a)) == 6  # 0 eager, 1 captured, 2 .. 5 replayed
    agent._noise_inject = fx.eps("r0")
    fixed = []
    for it in range(4):
        np.random.seed(7)
        r = agent.learn()
        fixed.append((r["critic_loss1"], r["actor_loss"]))
    assert len(set(fixed)) == 1 and fixed[0][0] not in c


@pytest.mark.parametrize("rows", [1, 5])
def test_act_draws_from_torch_normal_on_the_native_actor(rows):
    from jorldy_amd.core.agent import Agent

    S, A = 6, 3
    torch.manual_seed(0)
    agent = Agent("sac", state_size=S, action_size=A, hidden_size=64, buffer_size=64, batch_size=2, device="cuda")  # rows > batch_size: chunked forwards
    state = np.random.RandomState(3).randn(rows, S).astype(np.float32) * 2
    mu, std = agent.actor(agent.as_tensor(state))
    assert tuple(mu.shape) == tuple(std.shape) == (rows, A) and float(std.min()) >= np.exp(-1.0) * (1 - 1e-6) and float(std.max()) <= np.exp(1.0) * (1 + 1e-6)
    a64 = D.build(D.Actor, {k: v.cpu() for k, v in agent.actor.state_dict().items()}, torch.float64)
    with torch.no_grad():
        m64, s64 = a64(torch.from_numpy(state).double())
    margins.leq(float((mu.cpu().double() - m64).abs().max()), 1e-5, "mu vs the float64 actor")
    margins.leq(float((std.cpu().double() - s64).abs().max()), 1e-5, "std vs the float64 actor")
    torch.manual_seed(11)
    got = agent.act(state, True)["action"]
    torch.manual_seed(11)
    want = torch.tanh(torch.normal(mu, std)).cpu().numpy()
    assert got.shape == (rows, A) and got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(agent.act(state, False)["action"], torch.tanh(mu).cpu().numpy())
    x = agent.as_tensor(state)
    assert tuple(agent.critic1(x, torch.tanh(mu)).shape) == (rows, 1) and tuple(agent.target_critic2(x, torch.tanh(mu)).shape) == (rows, 1)


SAC_OPT = {"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}
SAC_KW = dict(actor="continuous_policy", critic="continuous_q_network", use_dynamic_alpha=True, gamma=0.99, tau=5e-3, buffer_size=64, static_log_alpha=-2.0, lr_decay=True)
SUPPORTED = [
    ("config.sac.mujoco", dict(state_size=11, action_size=3, batch_size=256, start_train_step=25000, optim_config=SAC_OPT, **SAC_KW)),
    ("config.sac.pendulum", dict(state_size=3, action_size=1, batch_size=64, start_train_step=5000, optim_config=SAC_OPT, **SAC_KW)),
    ("config.sac.cartpole", dict(state_size=4, action_size=1, batch_size=64, start_train_step=5000, target_update_period=500,
                                 optim_config=dict(SAC_OPT, actor_lr=1.5e-4, critic_lr=3e-4, alpha_lr=1e-5), **SAC_KW)),
    ("config.sac.hopper_mlagent", dict(state_size=19, action_size=3, batch_size=64, start_train_step=5000, optim_config=SAC_OPT, **SAC_KW)),
]


@pytest.mark.parametrize("label,kw", SUPPORTED, ids=[c[0] for c in SUPPORTED])
def test_reference_config_constructs_and_acts(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    agent = Agent("sac", device="cuda", **kw)
    assert agent._net.H == 512 and agent.action_type == "continuous" and agent.use_dynamic_alpha and agent.log_alpha == 0.0 and agent.alpha == 1.0
    assert agent.target_entropy == -kw["action_size"] and agent._net.get_alpha()["lr"] == np.float32(kw["optim_config"]["alpha_lr"])
    state = np.random.RandomState(0).randn(2, kw["state_size"]).astype(np.float32)
    for training in (True, False):
        a = agent.act(state, training)["action"]
        assert a.shape == (2, kw["action_size"]) and np.isfinite(a).all() and np.abs(a).max() <= 1.0
    with pytest.raises(ValueError, match="libjorldy_hip"):
        Agent("sac", device="cuda", **dict(kw, actor="discrete_policy", critic="discrete_q_network"))


@pytest.mark.parametrize("name", ["sac", "sac_odd"])
def test_checkpoint_and_weight_sync_roundtrip(name, tmp_path):
    fx = D.Fixture(load(name))
    a = _loaded_agent(fx)
    np.random.seed(3)
    for it in range(3):
        a.process([fx.buffer()[it]], it + 1)
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    want_keys = ["actor", "actor_optimizer", "critic1", "critic2", "critic_optimizer1", "critic_optimizer2"] + (["log_alpha", "alpha_optimizer"] if fx.dynamic else [])
    assert list(ckpt.keys()) == want_keys
    for net, okey in (("actor", "actor_optimizer"), ("critic1", "critic_optimizer1"), ("critic2", "critic_optimizer2")):
        assert tuple(ckpt[net].keys()) == (D.ACTOR_KEYS if net == "actor" else D.CRITIC_KEYS)
        params = [torch.nn.Parameter(v.clone()) for v in ckpt[net].values()]
        opt = torch.optim.Adam(params, lr=1e-3)
        opt.load_state_dict(ckpt[okey])  # the reference's format: torch.optim.Adam takes the state
        for p in params:
            assert opt.state[p]["exp_avg"].shape == p.shape and float(opt.state[p]["step"]) == 3.0
    blk = a._net.get_alpha()
    if fx.dynamic:
        p = torch.nn.Parameter(ckpt["log_alpha"].clone())
        opt = torch.optim.Adam([p], lr=1e-3)
        opt.load_state_dict(ckpt["alpha_optimizer"])
        assert tuple(p.shape) == (1,) and float(p.detach()) == blk["log_alpha"] and float(opt.state[p]["step"]) == 3.0 and float(opt.state[p]["exp_avg"]) == blk["m"]
        assert opt.param_groups[0]["lr"] == pytest.approx(float(fx.z["hyper/alpha_lr"]), rel=1e-6)
    # load(): critic 2 from "critic2", both targets equal their online nets, alpha in use = exp(loaded log_alpha), the alpha optimizer restored
    b = _agent_for(fx)
    b.load(str(tmp_path))
    for net in a._net.nets():
        assert torch.equal(a._net.flat(net), b._net.flat(net)), net
        assert torch.equal(a._net.flat(net, "m"), b._net.flat(net, "m")) and torch.equal(a._net.flat(net, "v"), b._net.flat(net, "v")), net
    assert torch.equal(b._net.critics["target"], b._net.critics["params"]) and not torch.equal(a._net.critics["target"], a._net.critics["params"])
    bb = b._net.get_alpha()
    for k in ("log_alpha", "m", "v", "step", "lr", "dynamic", "beta1", "beta2", "eps"):
        assert bb[k] == blk[k], k
    assert bb["alpha"] == float(np.float32(np.exp(np.float64(np.float32(blk["log_alpha"]))))) and (not fx.dynamic or bb["alpha"] != blk["alpha"])
    # sync_out / sync_in carry the actor only
    c = _agent_for(fx)
    before = c._net.critics["params"].clone()
    w = a.sync_out()["weights"]
    assert tuple(w.keys()) == D.ACTOR_KEYS and all(v.device.type == "cpu" for v in w.values())
    c.sync_in(w)
    assert torch.equal(c._net.actor["params"], a._net.actor["params"]) and torch.equal(c._net.critics["params"], before)
    # save_full / load_full: two more learns equal those of the uninterrupted agent bit for bit (log_alpha, alpha in use, the alpha moments)
    (tmp_path / "full").mkdir()
    with pytest.raises(ValueError, match="version 2 only"):
        a.save_full(str(tmp_path / "full"), version=1)
    assert os.listdir(str(tmp_path / "full")) == []
    a.save_full(str(tmp_path / "full"))
    d = _agent_for(fx)
    d.load_full(str(tmp_path / "full"))
    assert d.num_learn == a.num_learn == 3 and torch.equal(d._net.critics["target"], a._net.critics["target"])
    assert d._net.get_alpha() == dict(blk, coef=d._net.get_alpha()["coef"])
    rng = (np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state())
    want = [a.process([fx.buffer()[10 + it]], 4 + it) for it in range(2)]
    np.random.set_state(rng[0])
    torch.set_rng_state(rng[1])
    torch.cuda.set_rng_state(rng[2])
    got = [d.process([fx.buffer()[10 + it]], 4 + it) for it in range(2)]
    assert got == want, (got, want)
    assert torch.equal(_flat_state(d), _flat_state(a))
    da, aa = d._net.get_alpha(), a._net.get_alpha()
    assert da == aa, (da, aa)


# ----------------------------------------------------------------------------------------------- learning curve
CURVE_CONFIG = D.CURVE_CONFIG


def _curve_kwargs():
    c = CURVE_CONFIG
    t = c["sac"]
    return dict(state_size=c["S"], action_size=c["A"], hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"],
                run_step=c["run_step"], tau=c["tau"], gamma=c["gamma"], lr_decay=c["lr_decay"], use_dynamic_alpha=t["use_dynamic_alpha"],
                optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": t["actor_lr"], "critic_lr": t["critic_lr"], "alpha_lr": t["alpha_lr"]})


def _control_curve(agent, env, steps, chunk):
    """The single-mode loop (act, step, process([transition], step)) -> mean reward per `chunk` env steps."""
    out, acc = [], []
    state = env.obs().copy()
    for step in range(1, steps + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"], dtype=np.float32).reshape(1, -1))
        tr = {"state": state, "next_state": np.asarray(nxt, dtype=np.float32).copy(), "reward": np.asarray(rew, dtype=np.float64).reshape(1, 1),
              "done": np.asarray(done).astype(bool).reshape(1, 1)}
        tr.update(a)
        agent.process([tr], step)
        state = env.obs().copy()
        acc.append(float(np.asarray(rew).reshape(-1)[0]))
        if step % chunk == 0:
            out.append(float(np.mean(acc)))
            acc = []
    return out


def test_control_learning_curve_tracks_the_real_reference():
    """SAC with a dynamic temperature in the single-mode loop on the control env, three seeds, against the curves of the UNMODIFIED reference
    agent on the oracle's bit-identical env (tests/golden/curves_reference_sac.json, tools/gen_golden_sac.py).  Assertions as
    test_td3_gpu's curve test: both learn, and the ends lie within noise of each other."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curves_reference_sac.json")) as f:
        fx = json.load(f)
    c = CURVE_CONFIG
    assert fx["config"] == c, "the fixture was generated for another configuration: rerun tools/gen_golden_sac.py --only curves"
    ref = fx["sac"]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3

    def hip(seed):
        np.random.seed(seed)
        torch.manual_seed(seed)
        agent = Agent("sac", device="cuda", **_curve_kwargs())
        agent.memory.first_store = False
        return _control_curve(agent, ops.ControlVec(1, c["S"], c["A"], seed=1000 + seed), c["steps"], c["chunk"])

    g = [hip(s) for s in (1, 2, 3)]
    g_start, g_end = np.mean([x[0] for x in g]), np.mean([np.mean(x[-3:]) for x in g])
    r_start, r_end = np.mean([x[0] for x in ref]), np.mean([np.mean(x[-3:]) for x in ref])
    print(f"sac mean reward per step: HIP {g_start:.3f} -> {g_end:.3f}, reference {r_start:.3f} -> {r_end:.3f}")
    # the curves go beside the margin ledger (the scratch directory tests/margins.py writes to), before anything is asserted
    margins.record(abs(g_end - r_end), 0.25 * max(abs(r_end), 0.4), "sac: |end of the HIP curves - end of the reference's|")
    with open(os.path.join(os.path.dirname(margins.dump()), "learning_curve_sac_control.json"), "w") as f:
        json.dump({"config": c, "metric": fx["metric"], "hip": g, "reference": ref}, f)
    assert g_end > g_start + 0.3 and r_end > r_start + 0.3  # both learn (random play: ~0.1)
    assert abs(g_end - r_end) < 0.25 * max(abs(r_end), 0.4)
