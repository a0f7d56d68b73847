"""TD3 and DDPG on the GPU: the kernels of jh_td3.hip (Polyak average, next action, critic loss, actor seed, tanh backward) and the
network object (ops.ACNet) against the float64 truth of tests/td3_truth.py (pinned to the reference's own learn() by
tests/test_td3_cpu.py) and against the fixtures of tools/gen_golden_td3.py; then the whole agents: one learn() per fixture record with
the fixture's noise injected, hipGraph replay against eager over all three variants of TD3's learn(), acting in the reference's numpy
draw order, the configs' shapes, checkpoints, and the learning curves on the control env next to the reference's."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import td3_truth as D
from tests.util import f32, load, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5


# ----------------------------------------------------------------------------------------------- Polyak average
@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 270000])
def test_polyak_is_bit_identical_to_torch_on_float32_cpu_tensors(n):
    from jorldy_amd import ops

    rs = np.random.RandomState(n)
    p, t0 = torch.from_numpy(rs.randn(n).astype(np.float32)), torch.from_numpy(rs.randn(n).astype(np.float32))
    for tau in (0.0, 1e-3, 5e-3, 1.0):
        want = D.polyak(p, t0, tau)  # the reference's expression, evaluated by torch on float32 CPU tensors
        pd, td = p.cuda(), t0.clone().cuda()
        ops.td3_polyak(pd, td, tau)
        assert torch.equal(pd.cpu(), p), "params were written"
        assert np.array_equal(npy(td).view(np.uint32), want.numpy().view(np.uint32)), (n, tau)
        if tau == 1.0:
            assert torch.equal(td.cpu(), p)
        if tau == 0.0:
            assert torch.equal(td.cpu(), t0)
        # the same under graph replay: two replays are two updates
        td2 = t0.clone().cuda()
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            ops.td3_polyak(pd, td2, tau)
        td2.copy_(t0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(td2, td)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(npy(td2).view(np.uint32), D.polyak(p, want, tau).numpy().view(np.uint32))


# ----------------------------------------------------------------------------------------------- next action
@pytest.mark.parametrize("B,A", D.NEXT_ACTION_SHAPES)
def test_next_action_matches_float64_with_and_without_noise(B, A):
    from jorldy_amd import ops

    for z, eps in D.next_action_cases(B, A):
        got = ops.td3_next_action(f32(z), f32(eps), D.STD, D.CLIP)
        e = T.grad_vs_exact(npy(got), D.next_action(z, eps, D.STD, D.CLIP).numpy(), D.next_action(z, eps, D.STD, D.CLIP, torch.float32).numpy(), TOL, "next_action")
        plain = ops.td3_next_action(f32(z))
        e2 = T.grad_vs_exact(npy(plain), D.next_action(z, None, 0, 0).numpy(), D.next_action(z, None, 0, 0, torch.float32).numpy(), TOL, "tanh(z)")
        print(f"B{B} A{A}: |ours - fp64| / max = {e[0]:.3e} (noise), {e2[0]:.3e} (plain)")
        assert float(got.abs().max()) <= 1.0
        hi = (np.tanh(z.astype(np.float64)) + np.clip(eps.astype(np.float64) * D.STD, -D.CLIP, D.CLIP)) > 1.0 + 1e-6
        assert np.all(npy(got)[hi] == 1.0)


# ----------------------------------------------------------------------------------------------- critic loss, actor seed, tanh backward
@pytest.mark.parametrize("variant", D.CRITIC_LOSS_VARIANTS)
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("B", D.CRITIC_LOSS_B)
def test_critic_loss_matches_float64_truth(B, n, variant):
    from jorldy_amd import ops

    q, qn, r, d = D.critic_loss_case(B, n, variant)
    y, grad, st = ops.td3_critic_loss(f32(q), f32(qn), f32(r), f32(d), 0.99, stats=torch.full((4,), -1.0, device="cuda"))
    t, t32 = D.critic_loss(q, qn, r, d, 0.99), D.critic_loss(q, qn, r, d, 0.99, torch.float32)
    T.grad_vs_exact(npy(y), t["y"].numpy(), t32["y"].numpy(), TOL, "y")
    e = T.grad_vs_exact(npy(grad), t["grad"].numpy(), t32["grad"].numpy(), TOL, "d(loss_i)/d(q_i)")
    st = npy(st)
    assert st[3] == 0.0, "arrival mark"
    for i in range(n):
        np.testing.assert_allclose(st[i], float(t["loss"][i]), rtol=1e-5, err_msg=f"loss_{i + 1}")
    if n == 1:
        assert st[1] == 0.0
    np.testing.assert_allclose(st[2], float(t["max_Q"]), rtol=1e-5, err_msg="max_Q")
    print(f"B{B} n{n} {variant}: gradient |ours - fp64| / max = {e[0]:.3e}")


def test_critic_loss_is_bit_identical_across_runs_and_under_graph_replay():
    from jorldy_amd import ops

    for B, n in ((128, 2), (1025, 2), (7, 1)):
        args = [f32(a) for a in D.critic_loss_case(B, n, "plain", seed=1)]
        y1, g1, s1 = ops.td3_critic_loss(*args, 0.99)
        y2, g2, s2 = ops.td3_critic_loss(*args, 0.99)
        torch.cuda.synchronize()
        assert torch.equal(g1, g2) and torch.equal(s1, s2) and torch.equal(y1, y2)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with ops.graph_capture(graph):
            y3, g3, s3 = ops.td3_critic_loss(*args, 0.99)
        g3.fill_(7.0)
        s3.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g1, g3) and torch.equal(s1, s3) and torch.equal(y1, y3)


def test_critic_loss_rejects_out_of_range_sizes():
    from jorldy_amd import _lib, ops

    v = torch.zeros(4, device="cuda")
    for n in (0, 3):
        with pytest.raises(_lib.JhError, match="bad argument"):
            ops.td3_critic_loss(torch.zeros(n, 4, device="cuda"), torch.zeros(n, 4, device="cuda"), v, v, 0.99)
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.td3_critic_loss(torch.zeros(1, 0, device="cuda"), torch.zeros(1, 0, device="cuda"), v[:0], v[:0], 0.99)
    with pytest.raises(_lib.JhError, match="bad argument"):
        ops.td3_polyak(v, v.clone(), 1.5)


@pytest.mark.parametrize("B,A", [(1, 1), (7, 3), (128, 6), (1025, 17)])
def test_actor_seed_and_tanh_backward_match_float64(B, A):
    from jorldy_amd import ops

    rs = np.random.RandomState(B)
    q = rs.randn(B).astype(np.float32) * 3
    grad, st = ops.td3_actor_seed(f32(q), stats=torch.full((2,), -1.0, device="cuda"))
    t = D.actor_seed(q)
    st = npy(st)
    assert st[1] == 0.0
    np.testing.assert_allclose(st[0], float(t["actor_loss"]), rtol=1e-5, atol=1e-6 * float(np.abs(q).max()), err_msg="actor_loss")
    assert np.array_equal(npy(grad), np.full(B, np.float32(-1.0) / np.float32(B), np.float32))
    a, da = np.tanh(rs.randn(B, A) * 1.5).astype(np.float32), rs.randn(B, A).astype(np.float32)
    dz = ops.td3_tanh_backward(f32(da), f32(a))
    T.grad_vs_exact(npy(dz), da.astype(np.float64) * (1 - a.astype(np.float64) ** 2), da * (1 - a * a), TOL, "tanh backward")


# ----------------------------------------------------------------------------------------------- the network object
NET_SHAPES = [(3, 1, 32, 7), (11, 3, 64, 32), (17, 6, 256, 128), (4, 1, 512, 4)]


class Twin(torch.nn.Module):
    """The online critics as ONE module, so that fp64_truth.OptimTruth steps them with one torch.optim.Adam as the native object does."""

    def __init__(self, critics):
        super().__init__()
        self.c = torch.nn.ModuleList(critics)


def _mirrors(cls, S, A, H, seed):
    torch.manual_seed(seed)
    m = cls(S, A, H).double()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    T.round_to_fp32_(m)
    return m, T.as32(m)


def _twin_state(nat, kind):
    out = OrderedDict()
    for c in range(nat.nc):
        for k, v in nat.export_state(f"critic{c + 1}", kind).items():
            out[f"c.{c}.{k}"] = v
    return out


def _force_twin(nat, truth, lr, it):
    params, m, v = truth.teacher_force()
    for c in range(nat.nc):
        pick = lambda d: {k[len(f"c.{c}."):]: t for k, t in d.items() if k.startswith(f"c.{c}.")}
        nat.import_state(pick(params), f"critic{c + 1}")
        for kind, src in (("m", m), ("v", v)):
            if src is not None:
                nat.import_state(pick(src), f"critic{c + 1}", kind)
            else:
                nat.flat(f"critic{c + 1}", kind).zero_()
    nat.set_hyper("critic", lr, 0.9, 0.999, 1e-8, it)


def _force_actor(nat, truth, lr, it):
    params, m, v = truth.teacher_force()
    nat.import_state(params, "actor")
    for kind, src in (("m", m), ("v", v)):
        if src is not None:
            nat.import_state(src, "actor", kind)
        else:
            nat.flat("actor", kind).zero_()
    nat.set_hyper("actor", lr, 0.9, 0.999, 1e-8, it)


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("S,A,H,B", NET_SHAPES)
def test_acnet_forwards_critic_update_and_actor_update_match_float64(S, A, H, B, nc):
    from jorldy_amd import ops

    a64, a32 = _mirrors(D.Actor, S, A, H, 0)
    ta64, ta32 = _mirrors(D.Actor, S, A, H, 100)
    cs = [_mirrors(D.Critic, S, A, H, 1 + c) for c in range(nc)]
    tcs = [_mirrors(D.Critic, S, A, H, 101 + c) for c in range(nc)]
    tw64, tw32 = Twin([c[0] for c in cs]), Twin([c[1] for c in cs])
    nat = ops.ACNet(S, A, H, nc, B, "cuda:0")
    assert nat.nets() == ("actor", "critic1", "critic2")[: nc + 1]
    nat.import_state(a32.state_dict(), "actor")
    nat.import_state(ta32.state_dict(), "actor", "target")
    for c in range(nc):
        nat.import_state(cs[c][1].state_dict(), f"critic{c + 1}")
        nat.import_state(tcs[c][1].state_dict(), f"critic{c + 1}", "target")
    # ---- export / import round trip under the reference's keys
    sd = nat.export_state("actor")
    assert tuple(sd.keys()) == D.ACTOR_KEYS == tuple(a32.state_dict().keys())
    for k, v in a32.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k
    for c in range(nc):
        for kind, src in (("params", cs[c][1]), ("target", tcs[c][1])):
            sd = nat.export_state(f"critic{c + 1}", kind)
            assert tuple(sd.keys()) == D.CRITIC_KEYS
            for k, v in src.state_dict().items():
                assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), (c, kind, k)
    with pytest.raises(KeyError):
        nat.import_state({"head.l.weight": torch.zeros(H, S)}, "actor")
    # ---- every forward, online and target
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, generator=g)
    act = torch.tanh(torch.randn(B, A, generator=g))
    with torch.no_grad():
        for which, (m64, m32) in enumerate(((a64, a32), (ta64, ta32))):
            T.vs_exact(nat.actor_forward(x.cuda(), which), m64(x.double()), m32(x), TOL, f"actor forward which={which}")
        for which, nets in enumerate((cs, tcs)):
            q = nat.critic_forward(x.cuda(), act.cuda(), which)
            for c in range(nc):
                T.vs_exact(q[c], nets[c][0](x.double(), act.double()), nets[c][1](x, act), TOL, f"critic{c + 1} forward which={which}")
        if B > 1:
            T.vs_exact(nat.actor_forward(x[:1].cuda().contiguous(), 0), a64(x[:1].double()), a32(x[:1]), TOL, "actor forward, one row")
    # ---- the critic update: target pass, online pass, loss, backward, two teacher-forced Adam steps
    lr, gamma = 1e-3, 0.99
    truth = T.OptimTruth(tw64, tw32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    for it in range(2):
        _force_twin(nat, truth, lr, it)
        xa = torch.randn(2 * B, S, generator=g)
        act = torch.tanh(torch.randn(B, A, generator=g))
        r = torch.randn(B, generator=g)
        d = (torch.rand(B, generator=g) < 0.2).float()
        eps = torch.randn(B, A, generator=g) * 2 if nc == 2 else None
        stats, y, q = torch.full((4,), -1.0, device="cuda"), torch.empty(B, device="cuda"), torch.empty(nc, B, device="cuda")
        nat.critic_update(xa.cuda(), act.cuda(), r.cuda(), d.cuda(), None if eps is None else eps.cuda(), gamma, D.STD, D.CLIP, stats, y=y, q=q)
        ref = {}
        for dt, tw, ta_, tcs_ in ((torch.float64, tw64, ta64, [t[0] for t in tcs]), (torch.float32, tw32, ta32, [t[1] for t in tcs])):
            c = lambda t: t.to(dt)
            with torch.no_grad():
                a2 = D.next_action(ta_.pre(c(xa[B:])), None if eps is None else eps.numpy(), D.STD, D.CLIP, dt)
                yy = c(r).view(-1, 1) + (1 - c(d).view(-1, 1)) * gamma * torch.stack([tc(c(xa[B:]), a2) for tc in tcs_]).min(dim=0).values
            for p in tw.parameters():
                p.grad = None
            qs = [crit(c(xa[:B]), c(act)) for crit in tw.c]
            losses = [torch.nn.functional.mse_loss(yy, qq) for qq in qs]
            sum(losses).backward()
            ref[dt] = (yy, qs, losses)
        y64, q64, l64 = ref[torch.float64]
        y32, q32, l32 = ref[torch.float32]
        T.vs_exact(y, y64, y32, TOL, f"step {it} y")
        st = npy(stats)
        assert st[3] == 0.0
        for c in range(nc):
            T.vs_exact(q[c], q64[c].detach(), q32[c].detach(), TOL, f"step {it} q{c + 1}")
            T.vs_exact(torch.tensor(st[c]), l64[c].detach(), l32[c].detach(), TOL, f"step {it} critic_loss{c + 1}")
        T.vs_exact(torch.tensor(st[2]), y64.max(), y32.max(), TOL, f"step {it} max_Q")
        raw = _twin_state(nat, "grads")
        p32 = dict(tw32.named_parameters())
        for k, p in tw64.named_parameters():
            T.vs_exact(raw[k], p.grad, p32[k].grad, TOL, f"step {it} grad {k}")
        truth.step(None, raw, _twin_state(nat, "params"), _twin_state(nat, "m"), _twin_state(nat, "v"), tag=f"critic adam step {it}")
    # ---- the actor update: through critic 1's action input, the actor's Adam; critic 1 is not written
    atruth = T.OptimTruth(a64, a32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    for it in range(2):
        _force_actor(nat, atruth, lr, it)
        xs = torch.randn(B, S, generator=g)
        before = {kind: nat.critics[kind].clone() for kind in nat.KINDS}
        stats, a_pred = torch.full((2,), -1.0, device="cuda"), torch.empty(B, A, device="cuda")
        nat.actor_update(xs.cuda(), stats, action_pred=a_pred)
        torch.cuda.synchronize()
        for kind in nat.KINDS:
            assert torch.equal(nat.critics[kind], before[kind]), f"the actor update wrote the critics' {kind} bucket"
        sd_c1 = {k: v.cpu() for k, v in nat.export_state("critic1").items()}
        ref = {}
        for dt, actor in ((torch.float64, a64), (torch.float32, a32)):
            c1 = D.build(D.Critic, sd_c1, dt)
            for p in actor.parameters():
                p.grad = None
            a = actor(xs.to(dt))
            loss = -c1(xs.to(dt), a).mean()
            loss.backward()
            ref[dt] = (a.detach(), loss.detach())
        T.vs_exact(a_pred, ref[torch.float64][0], ref[torch.float32][0], TOL, f"actor step {it} actor(s)")
        st = npy(stats)
        assert st[1] == 0.0
        T.vs_exact(torch.tensor(st[0]), ref[torch.float64][1], ref[torch.float32][1], TOL, f"actor step {it} actor_loss")
        raw = nat.export_state("actor", "grads")
        p32 = dict(a32.named_parameters())
        for k, p in a64.named_parameters():
            T.vs_exact(raw[k], p.grad, p32[k].grad, TOL, f"actor step {it} grad {k}")
        atruth.step(None, raw, nat.export_state("actor"), nat.export_state("actor", "m"), nat.export_state("actor", "v"), tag=f"actor adam step {it}")
    # ---- soft update and target sync
    tau = 5e-3
    want = {net: {k: D.polyak(nat.export_state(net)[k].cpu(), nat.export_state(net, "target")[k].cpu(), tau) for k in nat.export_state(net)} for net in nat.nets()}
    nat.soft_update(tau)
    for net in nat.nets():
        for k, v in nat.export_state(net, "target").items():
            assert torch.equal(v.cpu(), want[net][k]), (net, k)
    nat.sync_target()
    for net in nat.nets():
        assert torch.equal(nat.flat(net, "target"), nat.flat(net))


# ----------------------------------------------------------------------------------------------- the agents
def _agent_for(fx, use_graph=True, **over):
    from jorldy_amd.core.agent import Agent

    z = fx.z
    kw = dict(state_size=fx.S, action_size=fx.A, hidden_size=fx.H, batch_size=fx.B, gamma=float(z["hyper/gamma"]), buffer_size=256, start_train_step=0,
              tau=float(z["hyper/tau"]), run_step=100000, device="cuda", use_graph=use_graph,
              optim_config={"actor": "adam", "critic": "adam", "actor_lr": float(z["hyper/actor_lr"]), "critic_lr": float(z["hyper/critic_lr"])})
    kw.update(over)
    return Agent(fx.kind, **kw)


def _net_of(fx_net):
    """fixture network name -> (ops.ACNet network, bucket)"""
    base = fx_net.replace("target_", "")
    return ("critic1" if base == "critic" else base), ("target" if fx_net.startswith("target_") else "params")


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


RECORDS = [(name, r) for name in D.FIXTURES for r in (("r0", "r1", "r2") if name.startswith("td3") else ("r0",))]


@pytest.mark.parametrize("name,r", RECORDS, ids=[f"{n}-{r}" for n, r in RECORDS])
def test_agent_learn_matches_the_reference_record(name, r):
    """One learn() from the fixture's starting state with num_learn, the numpy seed and the target noise as recorded: result keys and
    values (rtol 1e-5), y / q / actor(s), gradients, Adam moments, online weights within the caps of test_iqn_agent_learn_matches_reference
    (at most 0.5 % further than 2e-5 from the reference's, the worst within 2.1 lr), target weights within 2e-5; what the record says learn()
    left alone is bit-unchanged."""
    z = load(name)
    fx = D.Fixture(z)
    agent = _loaded_agent(fx)
    net = agent._net
    agent.num_learn = int(z[f"{r}/num_learn"])
    if fx.kind == "td3":
        agent._noise_inject = fx.eps(r)
        assert (agent.target_noise_std, agent.target_noise_clip, agent.update_delay) == (*fx.noise_args(), int(z["hyper/update_delay"]))
    start = {kind: (net.actor[kind].clone(), net.critics[kind].clone()) for kind in net.KINDS}
    np.random.seed(int(z["hyper/np_seed"]))
    result = agent.learn()
    torch.cuda.synchronize()
    keys = {"critic_loss1", "critic_loss2", "actor_loss", "max_Q"} if fx.kind == "td3" else {"critic_loss", "actor_loss", "max_Q"}
    assert set(result) == keys and agent.num_learn == int(z[f"{r}/num_learn"]) + 1
    for k in sorted(keys):
        print(f"{name} {r} result {k}: ours {result[k]!r} reference {float(z[f'{r}/result/{k}'])!r}")
        np.testing.assert_allclose(result[k], z[f"{r}/result/{k}"], rtol=1e-5, err_msg=k)
    st = agent._static
    b = fx.batch(r)
    assert np.array_equal(npy(st["tr"]["state"]), b["state"]) and np.array_equal(npy(st["tr"]["action"]), b["action"].astype(np.float32)), "other rows were sampled"
    np.testing.assert_allclose(npy(st["y"]), z[f"{r}/learn/target_q"].reshape(-1), rtol=1e-5, atol=1e-5, err_msg="y")
    np.testing.assert_allclose(npy(st["q"][0]), z[f"{r}/learn/q1"].reshape(-1), rtol=1e-5, atol=1e-5, err_msg="q1")
    if fx.kind == "td3":
        np.testing.assert_allclose(npy(st["q"][1]), z[f"{r}/learn/q2"].reshape(-1), rtol=1e-5, atol=1e-5, err_msg="q2")
    actor_step = fx.has_actor_step(r)
    if actor_step:
        np.testing.assert_allclose(npy(st["a_pred"]), z[f"{r}/learn/action_pred"], rtol=1e-5, atol=1e-5, err_msg="actor(s)")
    lrs = {"actor": float(z["hyper/actor_lr"]), "critic": float(z["hyper/critic_lr"])}
    tot = bad = 0
    worst = 0.0
    for fnet in fx.nets:
        onet, bucket = _net_of(fnet)
        ours = net.export_state(onet, bucket)
        if fx.unchanged(r, fnet):
            i, flat_now = (0, net.actor[bucket]) if onet == "actor" else (1, net.critics[bucket])
            lo = 0 if onet != "critic2" else net.n_critic
            hi = flat_now.numel() if onet == "actor" else lo + net.n_critic
            assert torch.equal(flat_now[lo:hi], start[bucket][i][lo:hi]), f"{fnet} changed where the reference's did not"
            continue
        if bucket == "target":
            for k, v in ours.items():
                margins.leq(float(np.abs(fx.thin(npy(v)) - z[f"{r}/sd1/{fnet}/{k}"]).max()), 2e-5, f"target weight {fnet} {k}")
            continue
        for k, v in net.export_state(onet, "grads").items():
            _cmp(fx, v, z[f"{r}/grad/{fnet}/{k}"], z[f"{r}/grad_absmax/{fnet}/{k}"], 1e-5, f"d(loss)/d {fnet} {k}")
        for kind, nm in (("m", "exp_avg"), ("v", "exp_avg_sq")):
            for k, v in net.export_state(onet, kind).items():
                ref = z[f"{r}/opt/{fnet}/{nm}/{k}"]
                _cmp(fx, v, ref, np.abs(ref).max(), 2e-5, f"{nm} {fnet} {k}")
        lr = lrs["actor" if onet == "actor" else "critic"]
        for k, v in ours.items():
            dd = np.abs(fx.thin(npy(v)) - z[f"{r}/sd1/{fnet}/{k}"])
            tot += dd.size
            bad += int((dd > 2e-5).sum())
            worst = max(worst, float(dd.max()) / lr)
    margins.leq(bad / tot, 0.005, "fraction of weights further than 2e-5 from the reference's")
    margins.leq(worst, 2.1, "worst weight difference / lr vs the possible travel")
    if not actor_step:
        assert fx.unchanged(r, "actor") and result["actor_loss"] == 0.0


def test_td3_graph_replay_equals_eager_over_all_three_variants():
    """Six consecutive learns with learning-rate decay between them: num_learn 0 (actor step, no soft update: eager warm-up), 1, 3, 5
    (critics only) and 2, 4 (actor step + soft update); both captured variants must exist afterwards."""
    fx = D.Fixture(load("td3"))
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent = _loaded_agent(fx, use_graph=use_graph, run_step=1000)
        np.random.seed(7)
        out, held = [], []
        for it in range(6):
            r = agent.learn()
            agent.learning_rate_decay(10 * (it + 1))
            out.append([r[k] for k in ("critic_loss1", "critic_loss2", "actor_loss", "max_Q")])
            held.append(sorted(agent._graphs))
        if use_graph:  # learn 0 eager (its variant never comes again), 1 and 2 captured, 3 onwards replayed
            assert held == [[], [(False, False)]] + [[(False, False), (True, True)]] * 4, f"captured variants, learn by learn: {held}"
        else:
            assert held == [[]] * 6
        res.append((out, torch.cat([agent._net.actor["params"], agent._net.actor["target"], agent._net.critics["params"], agent._net.critics["target"]]).clone()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)


def test_failed_capture_falls_back_to_eager(monkeypatch, capsys):
    """Four learns whose capture raises (before any stream enters capture) == four learns of an agent that never captures, bit for bit; the agent
    says so once, holds no graph and stays eager."""
    from jorldy_amd import ops
    from tests.util import refuse_capture

    monkeypatch.setattr(ops, "graph_capture", refuse_capture)
    fx = D.Fixture(load("td3"))
    res = []
    for use_graph in (True, False):
        torch.manual_seed(0)
        agent = _loaded_agent(fx, use_graph=use_graph, run_step=1000)
        np.random.seed(7)
        out = [agent.learn() for _ in range(4)]
        torch.cuda.synchronize()
        assert not agent._graphs and agent._learn_graphs.failed == use_graph
        res.append((out, torch.cat([agent._net.actor["params"], agent._net.actor["target"], agent._net.critics["params"], agent._net.critics["target"]]).clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    printed = capsys.readouterr().out
    assert printed.count("running eagerly") == 1
    assert "[jorldy_amd] hipGraph capture of TD3.learn() failed (RuntimeError: capture refused); running eagerly" in printed


def test_ddpg_graph_replay_equals_eager():
    fx = D.Fixture(load("ddpg"))
    res = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent = _loaded_agent(fx, use_graph=use_graph, run_step=1000)
        np.random.seed(7)
        out, held = [], []
        for it in range(4):
            r = agent.process([fx.buffer()[it]], 10 * (it + 1))  # learn + lr decay + the soft update of process()
            out.append([r[k] for k in ("critic_loss", "actor_loss", "max_Q")])
            held.append(sorted(agent._graphs))
        assert held == ([[]] + [[(True, False)]] * 3 if use_graph else [[]] * 4), f"captured variants, learn by learn: {held}"
        res.append((out, torch.cat([agent._net.actor["params"], agent._net.actor["target"], agent._net.critics["params"], agent._net.critics["target"]]).clone()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-6)


def test_replayed_learns_see_fresh_target_noise():
    """Learning rates 0, tau 0 and the same sampled rows: consecutive learns differ only in their target noise -- and so do the critic
    losses; with the noise injected they give the same bits."""
    fx = D.Fixture(load("td3"))
    torch.manual_seed(0)
    agent = _loaded_agent(fx, tau=0.0, lr_decay=False, optim_config={"actor": "adam", "critic": "adam", "actor_lr": 0.0, "critic_lr": 0.0})
    losses = []
    for it in range(7):
        np.random.seed(7)
        losses.append(agent.learn()["critic_loss1"])
    assert set(agent._graphs) == {(False, False), (True, True)}
    assert len(set(losses)) == 7  # 0 eager, 1 and 2 captured, 3 .. 6 replayed
    agent._noise_inject = fx.eps("r0")
    fixed = []
    for it in range(4):
        np.random.seed(7)
        fixed.append(agent.learn()["critic_loss1"])
    assert len(set(fixed)) == 1 and fixed[0] not in losses


def _actor64(agent):
    return D.build(D.Actor, {k: v.cpu() for k, v in agent.actor.state_dict().items()}, torch.float64)


def test_td3_act_follows_the_reference_draw_order():
    from jorldy_amd.core.agent import Agent

    S, A, rows, steps, n_random = 6, 3, 3, 40, 7
    torch.manual_seed(0)
    agent = Agent("td3", state_size=S, action_size=A, hidden_size=64, buffer_size=64, batch_size=8, initial_random_step=n_random, action_noise_std=0.8, device="cuda")
    a64 = _actor64(agent)
    rs = np.random.RandomState(3)
    states = [rs.randn(rows, S).astype(np.float32) * 2 for _ in range(steps)]
    np.random.seed(5)
    ours = [agent.act(s, True)["action"] for s in states]
    np.random.seed(5)
    n_clipped = 0
    for t, (s, a) in enumerate(zip(states, ours)):
        if t < n_random:  # td3.py:135-137: ONE uniform row whatever the number of rows
            assert a.shape == (1, A) and np.array_equal(a, np.random.uniform(-1.0, 1.0, (1, A))), t
            continue
        with torch.no_grad():
            mu = a64(torch.from_numpy(s).double()).numpy()
        noise = np.random.normal(0, 0.8, A)  # td3.py:142: ONE vector for all rows
        want = (mu + noise).clip(-1.0, 1.0)
        assert a.shape == (rows, A)
        margins.leq(float(np.abs(a - want).max()), 1e-5, "action vs float64 actor + the reference's noise draw")
        n_clipped += int((np.abs(mu + noise) > 1).sum())
    assert agent.num_random_step == n_random and n_clipped > 0
    state = np.random.get_state()
    ev = agent.act(states[0], False)["action"]  # evaluation: no noise, no draw
    with torch.no_grad():
        margins.leq(float(np.abs(ev - a64(torch.from_numpy(states[0]).double()).numpy()).max()), 1e-5, "evaluation action vs float64 actor")
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    # agent.actor / agent.critic1 are called as the reference's modules are
    x = agent.as_tensor(states[0])
    q = agent.critic1(x, agent.actor(x))
    assert tuple(q.shape) == (rows, 1) and tuple(agent.target_critic2(x, agent.target_actor(x)).shape) == (rows, 1)


def test_ddpg_act_follows_the_reference_draw_order():
    from jorldy_amd.core.agent import Agent

    S, A, rows, steps = 5, 2, 3, 40
    mu0, theta, sigma = 0.1, 0.15, 0.9
    torch.manual_seed(0)
    agent = Agent("ddpg", state_size=S, action_size=A, hidden_size=64, buffer_size=64, batch_size=8, mu=mu0, theta=theta, sigma=sigma, device="cuda")
    a64 = _actor64(agent)
    rs = np.random.RandomState(3)
    states = [rs.randn(rows, S).astype(np.float32) * 2 for _ in range(steps)]
    assert agent.OU.X.dtype == np.float32 and agent.OU.X.shape == (1, A)
    np.random.seed(5)
    ours = [agent.act(s, True)["action"] for s in states]
    assert agent.OU.X.dtype == np.float64
    np.random.seed(5)
    X = np.ones((1, A), dtype=np.float32) * mu0
    n_clipped = n_outside = 0
    for s, a in zip(states, ours):
        X = X + (theta * (mu0 - X) + sigma * np.random.randn(1))  # utils.py:21-24: ONE draw for all action dimensions
        with torch.no_grad():
            mu = a64(torch.from_numpy(s).double()).numpy()
        want = mu + X.clip(-1.0, 1.0)  # ddpg.py:114: only the noise is clipped
        assert a.shape == (rows, A)
        margins.leq(float(np.abs(a - want).max()), 1e-5, "action vs float64 actor + the reference's OU draw")
        n_clipped += int((np.abs(X) > 1).sum())
        n_outside += int((np.abs(a) > 1).sum())
    assert n_clipped > 0 and n_outside > 0
    np.testing.assert_allclose(agent.OU.X, X, rtol=0, atol=0)
    ev = agent.act(states[0], False)["action"]
    with torch.no_grad():
        margins.leq(float(np.abs(ev - a64(torch.from_numpy(states[0]).double()).numpy()).max()), 1e-5, "evaluation action vs float64 actor")
    np.testing.assert_allclose(agent.OU.X, X, rtol=0, atol=0)


TD3_OPT = {"actor": "adam", "critic": "adam", "actor_lr": 1e-3, "critic_lr": 1e-3}
DDPG_OPT = {"actor": "adam", "critic": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3}
DDPG_KW = dict(actor="deterministic_policy", critic="continuous_q_network", gamma=0.99, buffer_size=64, batch_size=128, tau=1e-3, lr_decay=True, mu=0, theta=1e-3, sigma=2e-3)
SUPPORTED = [
    ("config.td3.mujoco", "td3", dict(state_size=11, action_size=3, actor="deterministic_policy", critic="continuous_q_network", hidden_size=512, gamma=0.99,
                                      buffer_size=64, batch_size=128, start_train_step=25000, initial_random_step=25000, tau=5e-3, update_delay=2, action_noise_std=0.1,
                                      target_noise_std=0.2, target_noise_clip=0.5, lr_decay=True,
                                      optim_config={"actor": "adam", "critic": "adam", "actor_lr": 3e-4, "critic_lr": 3e-4}), 512),
    ("config.td3.cartpole", "td3", dict(state_size=4, action_size=1, actor="deterministic_policy", critic="continuous_q_network", gamma=0.99, buffer_size=64,
                                        batch_size=128, start_train_step=1000, initial_random_step=0, tau=1e-3, actor_period=2, act_noise_std=0.1, target_noise_std=0.2,
                                        target_noise_clip=0.5, lr_decay=True, optim_config=TD3_OPT), 256),
    ("config.ddpg.mujoco", "ddpg", dict(state_size=11, action_size=3, start_train_step=1000, optim_config=DDPG_OPT, **DDPG_KW), 512),
    ("config.ddpg.pendulum", "ddpg", dict(state_size=3, action_size=1, start_train_step=2000, optim_config=DDPG_OPT, **DDPG_KW), 512),
    ("config.ddpg.cartpole", "ddpg", dict(state_size=4, action_size=1, start_train_step=2000, optim_config=DDPG_OPT, **DDPG_KW), 512),
    ("config.ddpg.hopper_mlagent", "ddpg", dict(state_size=19, action_size=3, start_train_step=2000, optim_config=DDPG_OPT, **DDPG_KW), 512),
]


@pytest.mark.parametrize("label,name,kw,H", SUPPORTED, ids=[c[0] for c in SUPPORTED])
def test_reference_config_constructs_and_acts(label, name, kw, H):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    agent = Agent(name, device="cuda", **kw)
    assert agent._net.H == H and agent.action_type == "continuous"
    if label == "config.td3.cartpole":  # the stray keys are swallowed: the defaults apply (td3.py:62-63)
        assert agent.update_delay == 2 and agent.action_noise_std == 0.1 and not hasattr(agent, "actor_period") and not hasattr(agent, "act_noise_std")
    S, A = kw["state_size"], kw["action_size"]
    state = np.random.randn(2, S).astype(np.float32)
    for training in (True, False):
        a = agent.act(state, training)["action"]
        random_phase = name == "td3" and training and kw.get("initial_random_step", 0) > 0
        assert a.shape == ((1, A) if random_phase else (2, A)) and np.isfinite(a).all()


def test_unsupported_configurations_raise_at_construction():
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.ddpg import DDPG_ELIGIBLE
    from jorldy_amd.core.agent.td3 import TD3_ELIGIBLE

    base = dict(state_size=4, action_size=2, device="cuda")
    for name, text in (("td3", TD3_ELIGIBLE), ("ddpg", DDPG_ELIGIBLE)):
        for over in (dict(head="cnn", state_size=(4, 84, 84)), dict(state_size=(4,)), dict(hidden_size=30), dict(optim_config=dict(TD3_OPT, actor="rmsprop")),
                     dict(optim_config=dict(TD3_OPT, critic="sgd")), dict(optim_config=dict(TD3_OPT, weight_decay=0.1))):
            with pytest.raises(ValueError) as e:
                Agent(name, **dict(base, **over))
            assert text in str(e.value), (name, over)


@pytest.mark.parametrize("name", ["td3", "ddpg"])
def test_checkpoint_and_weight_sync_roundtrip(name, tmp_path):
    fx = D.Fixture(load(name))
    a = _loaded_agent(fx)
    np.random.seed(3)
    for _ in range(3):
        a.learn()  # TD3: actor steps at num_learn 0 and 2, a soft update at 2; the checkpoint carries moments and step counts
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    want_keys = (["actor", "actor_optimizer", "critic1", "critic2", "critic_optimizer1", "critic_optimizer2"] if name == "td3"
                 else ["actor", "actor_optimizer", "critic", "critic_optimizer"])
    assert list(ckpt.keys()) == want_keys
    for net, okey, steps in [("actor", "actor_optimizer", 2 if name == "td3" else 3)] + [(k, k.replace("critic", "critic_optimizer"), 3) for k in want_keys if k.startswith("critic") and "opt" not in k]:
        assert tuple(ckpt[net].keys()) == (D.ACTOR_KEYS if net == "actor" else D.CRITIC_KEYS)
        params = [torch.nn.Parameter(v.clone()) for v in ckpt[net].values()]
        opt = torch.optim.Adam(params, lr=1e-3)
        opt.load_state_dict(ckpt[okey])  # the reference's format: torch.optim.Adam takes the state
        for p in params:
            assert opt.state[p]["exp_avg"].shape == p.shape and opt.state[p]["exp_avg_sq"].shape == p.shape and float(opt.state[p]["step"]) == float(steps)
    b = _agent_for(fx)
    b.load(str(tmp_path))
    b.memory.first_store = False
    b.memory.store(fx.buffer())
    for net in a._net.nets():  # critic 2 from "critic2"; every target equals its loaded online network
        assert torch.equal(a._net.flat(net), b._net.flat(net)) and torch.equal(b._net.flat(net, "target"), b._net.flat(net)), net
        assert torch.equal(a._net.flat(net, "m"), b._net.flat(net, "m")) and torch.equal(a._net.flat(net, "v"), b._net.flat(net, "v")), net
    a._net.sync_target()  # what load() leaves: the next learn() of both starts from the same state
    a.num_learn = b.num_learn = 4
    res = []
    for ag in (a, b):
        np.random.seed(11)
        ag._noise_inject = fx.eps("r0")
        res.append(ag.learn())
        ag._noise_inject = None
    for k in res[0]:
        np.testing.assert_allclose(res[1][k], res[0][k], rtol=1e-6, err_msg=k)
    flat = lambda ag: torch.cat([ag._net.actor["params"], ag._net.critics["params"], ag._net.actor["target"], ag._net.critics["target"]])
    torch.testing.assert_close(flat(b), flat(a), rtol=1e-5, atol=1e-6)
    # sync_out / sync_in carry the actor only
    c = _agent_for(fx)
    before = c._net.critics["params"].clone()
    w = a.sync_out()["weights"]
    assert tuple(w.keys()) == D.ACTOR_KEYS and all(v.device.type == "cpu" for v in w.values())
    c.sync_in(w)
    assert torch.equal(c._net.actor["params"], a._net.actor["params"]) and torch.equal(c._net.critics["params"], before)
    # save_full / load_full: buffer, counters, actor_loss, targets, exploration state and the RNG states survive
    if name == "ddpg":
        a.act(np.zeros((1, fx.S), np.float32), True)  # the OU state leaves its initial value
    else:
        a.num_random_step = 5
    (tmp_path / "full").mkdir()
    with pytest.raises(ValueError, match="version 2 only"):  # the single-pickle format would drop the exploration state
        a.save_full(str(tmp_path / "full"), version=1)
    assert os.listdir(str(tmp_path / "full")) == []
    a.save_full(str(tmp_path / "full"))
    want = a.learn()
    d = _agent_for(fx)
    d.load_full(str(tmp_path / "full"))
    assert d.num_learn == a.num_learn - 1 and d.actor_loss == res[0]["actor_loss"]
    if name == "ddpg":
        assert np.array_equal(d.OU.X, a.OU.X) and d.OU.X.dtype == a.OU.X.dtype
    else:
        assert d.num_random_step == 5
    got = d.learn()
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-6, err_msg=f"load_full {k}")


# ----------------------------------------------------------------------------------------------- learning curves
CURVE_CONFIG = dict(S=11, A=3, steps=8000, chunk=1000, run_step=10000, hidden=256, batch=128, buffer=50000, start=1000, tau=5e-3, gamma=0.99, lr_decay=True,
                    td3=dict(initial_random_step=1000, actor_lr=1e-3, critic_lr=1e-3), ddpg=dict())


def _curve_kwargs(kind):
    c = CURVE_CONFIG
    kw = dict(state_size=c["S"], action_size=c["A"], hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"],
              run_step=c["run_step"], tau=c["tau"], gamma=c["gamma"], lr_decay=c["lr_decay"])
    if kind == "td3":
        t = c["td3"]
        kw.update(initial_random_step=t["initial_random_step"], optim_config={"actor": "adam", "critic": "adam", "actor_lr": t["actor_lr"], "critic_lr": t["critic_lr"]})
    return kw


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


@pytest.mark.parametrize("kind", ["td3", "ddpg"])
def test_control_learning_curve_tracks_the_real_reference(kind):
    """TD3 / DDPG in the single-mode loop on the control env, three seeds, against the curves of the UNMODIFIED reference agents on the
    oracle's bit-identical env (tests/golden/curves_reference_td3.json, tools/gen_golden_td3.py).  Assertions as
    test_ppo_continuous_control_learning_curve_tracks_the_real_reference: both learn, and the ends lie within noise of each other."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "curves_reference_td3.json")) as f:
        fx = json.load(f)
    c = CURVE_CONFIG
    assert fx["config"] == c, "the fixture was generated for another configuration: rerun tools/gen_golden_td3.py --only curves"
    ref = fx[kind]["reference"]
    assert fx["seeds"] == [1, 2, 3] and len(ref) == 3

    def hip(seed):
        np.random.seed(seed)
        torch.manual_seed(seed)
        agent = Agent(kind, device="cuda", **_curve_kwargs(kind))
        agent.memory.first_store = False
        return _control_curve(agent, ops.ControlVec(1, c["S"], c["A"], seed=1000 + seed), c["steps"], c["chunk"])

    g = [hip(s) for s in (1, 2, 3)]
    g_start, g_end = np.mean([x[0] for x in g]), np.mean([np.mean(x[-3:]) for x in g])
    r_start, r_end = np.mean([x[0] for x in ref]), np.mean([np.mean(x[-3:]) for x in ref])
    print(f"{kind} mean reward per step: HIP {g_start:.3f} -> {g_end:.3f}, reference {r_start:.3f} -> {r_end:.3f}")
    # the curves go beside the margin ledger (the scratch directory tests/margins.py writes to), before anything is asserted
    margins.record(abs(g_end - r_end), 0.25 * max(abs(r_end), 0.4), f"{kind}: |end of the HIP curves - end of the reference's|")
    with open(os.path.join(os.path.dirname(margins.dump()), f"learning_curve_{kind}_control.json"), "w") as f:
        json.dump({"config": c, "metric": fx["metric"], "hip": g, "reference": ref}, f)
    assert g_end > g_start + 0.3 and r_end > r_start + 0.3  # both learn (random play: ~0.1)
    assert abs(g_end - r_end) < 0.25 * max(abs(r_end), 0.4)
