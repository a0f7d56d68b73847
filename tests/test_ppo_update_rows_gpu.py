"""jh_pponet_ppo_update_rows (PPONet.ppo_update_rows: what the PPO agent calls for every minibatch the four-launch update does not take) across
every dispatch boundary inside it -- the case table, the input generator and its conditions: tests/ppo_update_cases.py.

  a. against a float64 evaluation of the same update (tests/fp64_truth.py: ppo_update_float64; torch-CPU-fp32 beside it): heads, statistics,
     every parameter's raw gradient, the clip coefficient, the stepped weights and the moments
  b. bit for bit against the path it replaces (forward -> ppo_loss_*, two-pass above 1024 rows -> backward -> adam_step), by the consumer's
     reduction of the loss partials and by the ticket's; with the norm folded into the dW1 launches: to fp32 rounding
  c. state carried from one call to the next (ticket word, partials, dv2 / mix / g_all columns, norm slots), eager and under graph capture
  d. the agent reaches these shapes: a learn() with 2048 + 1042-row minibatches at hidden 64

Criteria are the project's own: fp64_truth.vs_exact (1e-5 or twice torch-CPU-fp32's error, of the tensor's largest entry), BASELINE's 1e-5 on
|ours - exact| / (1 + |exact|) for the loss scalars, rtol 2e-5 on max_ratio / min_prob, the per-element Adam bound of fp64_truth."""
import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import ppo_update_cases as PC
from tests.util import npy

pytestmark = pytest.mark.gpu

STAT_KEYS = ("loss", "actor", "critic", "entropy", "max_ratio", "min_prob", "c1", "c2")
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def _dev(inp):
    d = {k: inp[k].cuda() for k in ("x", "action", "adv", "ret", "value_old", "logp_old")}
    d["idx"] = inp["idx"].cuda() if inp["idx"] is not None else None
    return d


def _flat(module):
    return torch.cat([p.detach().float().reshape(-1) for p in module.parameters()]).cuda()


def _unflat(flat, module):
    out, o = {}, 0
    for k, p in module.named_parameters():
        out[k] = flat[o : o + p.numel()].view_as(p)
        o += p.numel()
    return out


def _net(c, p0, max_rows=None, step=0.0, m=None, v=None):
    from jorldy_amd import ops

    # (row capacity as the agent sizes it: whole 256-row blocks above the minibatch, never exactly B)
    net = ops.PPONet(c.S, c.H, c.A, c.cont, max_rows or ((c.B + 255) // 256 + 1) * 256, "cuda:0")
    assert net.n_params == p0.numel()
    net.params.copy_(p0)
    if m is not None:
        net.m.copy_(m)
        net.v.copy_(v)
    net.set_hyper(PC.LR, B1, B2, ADAM_EPS, step=step)
    return net


def _n_params(c):
    from jorldy_amd import _lib as L

    return int(L.load().jh_pponet_param_count(c.S, c.H, c.A, int(c.cont)))


def _update(net, d, hyp, max_norm, stats, do_adam=True):
    eps, vf, ent = hyp
    net.ppo_update_rows(d["x"], d["idx"], d["action"], d["adv"], d["ret"], d["value_old"], d["logp_old"], eps, vf, ent, max_norm, stats, do_adam=do_adam)


def _separate(net, cont, d, hyp, max_norm, stats):
    """The path ppo_update_rows replaces: the public calls one after the other (ppo_loss_*: the two-pass kernels above 1024 rows)."""
    from jorldy_amd import ops

    eps, vf, ent = hyp
    if cont:
        mu, ls, vp = net.forward(d["x"], idx=d["idx"])
        g_mu, g_ls, g_v, _ = ops.ppo_loss_continuous(mu, ls, vp, d["idx"], d["action"], d["adv"], d["ret"], d["value_old"], d["logp_old"], eps, vf, ent, stats=stats)
        net.backward(d["x"], d["idx"], g_mu, g_ls, g_v)
    else:
        z, vp = net.forward(d["x"], idx=d["idx"])
        g_z, g_v, _ = ops.ppo_loss_discrete(z, vp, d["idx"], d["action"], d["adv"], d["ret"], d["value_old"], d["logp_old"], eps, vf, ent, stats=stats)
        net.backward(d["x"], d["idx"], g_z, None, g_v)
    net.adam_step(max_norm)


def _state(net, stats):
    torch.cuda.synchronize()
    return {"statistics": npy(stats).copy(), "gradient bucket": npy(net.grads).copy(), "weights": npy(net.params).copy(), "exp_avg": npy(net.m).copy(), "exp_avg_sq": npy(net.v).copy()}


def _assert_same_bits(a, b, what):
    for k in a:
        diff = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
        assert np.array_equal(a[k], b[k]), f"{what}: {k} differ in {int((a[k] != b[k]).sum())} of {a[k].size} entries (max |diff| {np.nanmax(diff):.3e}, max |entry| {np.abs(b[k]).max():.3e})"


@pytest.mark.parametrize("c", PC.CASES, ids=PC.IDS)
def test_ppo_update_rows_vs_float64(c):
    """(a) one ppo_update_rows(do_adam=False) -> statistics row + raw gradient bucket; a fresh net with do_adam=True -> clipped gradient (the call has
    no norm output: the clip coefficient is read off as clipped / raw), weights, moments."""
    inp = PC.make(c)
    exact = PC.truth(c, inp)
    print(PC.case_id(c), PC.check_conditions(c, inp, exact))  # conditions on the reference alone: before anything touches the GPU
    ref32 = PC.truth(c, inp, T.as32(inp["module"]))
    module, hyp, tag = inp["module"], (inp["eps"], inp["vf"], inp["ent"]), PC.case_id(c)
    d, p0 = _dev(inp), _flat(inp["module"])
    # ---- heads (the forward inside the call, by itself), statistics, raw gradient
    net = _net(c, p0)
    outs = net.forward(d["x"], idx=d["idx"])
    for nm, a, b, r in zip(("mu", "log_std", "value") if c.cont else ("logits", "value"), outs, exact[0], ref32[0]):
        T.vs_exact(a, b, r, 1e-5, f"{tag} head {nm}")
    st = torch.full((8,), -1.0, device="cuda")
    _update(net, d, hyp, c.max_norm, st, do_adam=False)
    torch.cuda.synchronize()
    s = st.double().cpu()
    for j, k in enumerate(STAT_KEYS):
        e = exact[1][k]
        print(f"  {k}: ours {float(s[j]):.9g} float64 {e:.9g} torch-cpu-fp32 {ref32[1][k]:.9g}")
        if k in ("max_ratio", "min_prob"):
            margins.close(float(s[j]), e, rtol=2e-5, what=f"{tag} {k}")
        else:
            margins.leq(abs(float(s[j]) - e) / (1.0 + abs(e)), 1e-5, f"{tag} {k}: |ours - fp64| / (1 + |fp64|)")
    raw = net.grads.clone()
    ours_g = _unflat(raw, module)
    for k in exact[2]:
        T.vs_exact(ours_g[k], exact[2][k], ref32[2][k], 1e-5, f"{tag} grad {k}")
    # ---- clip + Adam in the same call
    net2 = _net(c, p0)
    st2 = torch.full((8,), -1.0, device="cuda")
    _update(net2, d, hyp, c.max_norm, st2, do_adam=True)
    torch.cuda.synchronize()
    assert torch.equal(st2, st), "the statistics row depends on do_adam"
    norm64 = float(torch.sqrt((raw.double() ** 2).sum()))  # float64 norm of OUR raw gradient
    coef = min(1.0, c.max_norm / (norm64 + 1e-6)) if c.max_norm > 0 else 1.0
    big = raw.abs() > 0.1 * raw.abs().max()
    margins.close(npy(net2.grads.double()[big] / raw.double()[big]), coef, rtol=1e-5, what=f"{tag} clip coefficient (clipped / raw), norm {norm64:.4g} vs max_norm {c.max_norm:g}")
    margins.leq(float((net2.grads.double() - coef * raw.double()).abs().max()), 1e-5 * coef * float(raw.abs().max()), f"{tag} clipped bucket vs coefficient x raw bucket")
    T.check_first_step_from_our_gradient({"bucket": p0}, {"bucket": net2.grads}, {"bucket": net2.params},
                                         lambda ps: torch.optim.Adam(ps, lr=PC.LR, betas=(B1, B2), eps=ADAM_EPS), PC.LR, f"{tag} Adam's first step")
    g = net2.grads.double()
    for nm, ours, ex in (("exp_avg", net2.m, (1.0 - B1) * g), ("exp_avg_sq", net2.v, (1.0 - B2) * g * g)):
        margins.leq(float((ours.double() - ex).abs().max()), 1e-5 * float(ex.abs().max()) + 1e-30, f"{tag} {nm} vs float64 step of OUR gradient, / max")


@pytest.mark.parametrize("c", PC.CASES, ids=PC.IDS)
def test_ppo_update_rows_is_bit_identical_to_the_separate_calls(c, monkeypatch):
    """(b) the C source's promise at every case of (a): same statistics, gradient bucket, weights and moments as forward -> ppo_loss_* -> backward ->
    adam_step, whoever reduces the loss partials.  The "tail" cases put the critic's branch into the hands of the last loss workgroup: one row taking
    the other branch's value gradient changes bits here even where (a)'s tolerance would hide it."""
    inp = PC.make(c)
    hyp, tag = (inp["eps"], inp["vf"], inp["ent"]), PC.case_id(c)
    d, p0 = _dev(inp), _flat(inp["module"])
    st = [torch.full((8,), -1.0, device="cuda") for _ in range(4)]
    n0 = _net(c, p0)
    _separate(n0, c.cont, d, hyp, c.max_norm, st[0])
    s0 = _state(n0, st[0])
    monkeypatch.setenv("JH_PPO_NORM_FOLD", "0")
    n1 = _net(c, p0)
    _update(n1, d, hyp, c.max_norm, st[1])
    s1 = _state(n1, st[1])
    monkeypatch.setenv("JH_PPO_LOSS_TICKET", "1")
    n2 = _net(c, p0)
    _update(n2, d, hyp, c.max_norm, st[2])
    s2 = _state(n2, st[2])
    monkeypatch.delenv("JH_PPO_LOSS_TICKET")
    monkeypatch.delenv("JH_PPO_NORM_FOLD")
    n3 = _net(c, p0)
    _update(n3, d, hyp, c.max_norm, st[3])
    s3 = _state(n3, st[3])
    _assert_same_bits(s2, s0, f"{tag}: one call (ticket) vs the separate calls")
    _assert_same_bits(s1, s0, f"{tag}: one call vs the separate calls")
    # the norm folded into the dW1 launches: another order of the same additions (test_ppo_norm_folded_into_the_dw1_launches_equals_the_norm_kernel's bounds)
    f64 = lambda a: a.astype(np.float64)
    margins.leq(float(np.abs(f64(s3["statistics"]) - f64(s0["statistics"])).max() / (1.0 + np.abs(s0["statistics"]).max())), 1e-6, f"{tag}: statistics, folded norm vs norm kernel")
    margins.leq(float(np.abs(f64(s3["gradient bucket"]) - f64(s0["gradient bucket"])).max() / np.abs(s0["gradient bucket"]).max()), 1e-6, f"{tag}: clipped gradient, folded norm vs norm kernel")
    margins.leq(float(np.abs(f64(s3["weights"]) - f64(s0["weights"])).max()), 1e-7 + 1e-2 * PC.LR, f"{tag}: weights, folded norm vs norm kernel")


def _random_rollout(cont, S, A, M, seed):
    """Unstructured inputs (bit identity needs no well-defined truth)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, S, generator=g)
    action = torch.tanh(torch.randn(M, A, generator=g)) if cont else torch.randint(0, A, (M, 1), generator=g).float()
    adv, ret, vold = (torch.randn(M, 1, generator=g) for _ in range(3))
    logp_old = -torch.rand(M, A if cont else 1, generator=g) - 0.3
    return {"x": x.cuda(), "action": action.cuda(), "adv": adv.cuda(), "ret": ret.cuda(), "value_old": vold.cuda(), "logp_old": logp_old.cuda()}, g


@pytest.mark.parametrize("cont", [False, True])
def test_ppo_update_rows_carries_no_state_between_calls(cont, monkeypatch):
    """(c) one net through B = 20 000 -> 300 -> 1030 -> 2048 -> 7 with the ticket switch alternating: every call equals, bit for bit, the same call on a
    fresh net given the same weights, moments and step -- the ticket word is left at zero, nothing stale is read from the partials, dv2, mix, the g_all
    columns or the norm slots of an earlier, larger call."""
    c = PC.Case(cont, 11 if cont else 4, 64, 3 if cont else 2, 20000, 21000, "-", 0.5)
    hyp = PC.hyper(c)
    roll, g = _random_rollout(cont, c.S, c.A, c.M, 11)
    p0 = torch.randn(_n_params(c), generator=g).cuda() * (0.7 / np.sqrt(c.H))
    net = _net(c, p0)
    for k, (B, ticket) in enumerate(zip((20000, 300, 1030, 2048, 7), ("0", "1", "0", "1", "0"))):
        monkeypatch.setenv("JH_PPO_LOSS_TICKET", ticket)
        d = dict(roll, idx=torch.randperm(c.M, generator=g)[:B].cuda())
        before = (net.params.clone(), net.m.clone(), net.v.clone())
        st, st_f = torch.full((8,), -1.0, device="cuda"), torch.full((8,), -1.0, device="cuda")
        _update(net, d, hyp, c.max_norm, st)
        fresh = _net(c._replace(B=B), before[0], step=float(k), m=before[1], v=before[2])
        _update(fresh, d, hyp, c.max_norm, st_f)
        _assert_same_bits(_state(net, st), _state(fresh, st_f), f"call {k} (B = {B}, JH_PPO_LOSS_TICKET={ticket}) vs a fresh net")


@pytest.mark.parametrize("cont", [False, True])
def test_ppo_update_rows_graph_replay_equals_eager(cont):
    """(c) the agent captures whole learns: B = 1030 then B = 2048 in ONE captured graph, replayed twice, against the same four calls issued eagerly
    (default hardware queues)."""
    from jorldy_amd import ops

    c = PC.Case(cont, 11 if cont else 4, 64, 3 if cont else 2, 2048, 3000, "-", 0.5)
    hyp = PC.hyper(c)
    roll, g = _random_rollout(cont, c.S, c.A, c.M, 12)
    p0 = torch.randn(_n_params(c), generator=g).cuda() * (0.7 / np.sqrt(c.H))
    ds = [dict(roll, idx=torch.randperm(c.M, generator=g)[:B].cuda()) for B in (1030, 2048)]

    def enqueue(net, stats):
        for k, d in enumerate(ds):
            _update(net, d, hyp, c.max_norm, stats[k])

    def reset(net):
        net.params.copy_(p0)
        net.m.zero_()
        net.v.zero_()
        net.set_hyper(PC.LR, B1, B2, ADAM_EPS, step=0.0)

    ne, ng = _net(c, p0), _net(c, p0)
    st_e, st_g = torch.full((2, 8), -1.0, device="cuda"), torch.full((2, 8), -1.0, device="cuda")
    enqueue(ng, st_g)  # warm-up (first-use allocations), then back to the start
    reset(ng)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        enqueue(ng, st_g)
    for rep in range(2):
        graph.replay()
        enqueue(ne, st_e)
        _assert_same_bits(_state(ng, st_g), _state(ne, st_e), f"replay {rep} vs eager")


@pytest.mark.parametrize("cont,S,A", [(False, 4, 2), (True, 17, 6)])
def test_ppo_agent_learn_with_ragged_wide_minibatches_one_call_equals_separate_calls(cont, S, A, monkeypatch):
    """(d) Agent("ppo").learn() at hidden 64 on 3 x 1030 generated rows with batch_size 2048: minibatches of 2048 and 1042 rows (1042 x 16 % 64 = 32: a
    partial last wave in the backward's first kernel), 2 + 1 discrete outputs and 13 continuous ones; JH_PPO_ONEPASS 0 vs 1, the norm kernel in both."""
    from jorldy_amd.core.agent import Agent
    from oracle import synth

    W, Tn, H, E, lr = 3, 1030, 64, 2, 3e-4
    M = W * Tn
    monkeypatch.setenv("JH_PPO_NORM_FOLD", "0")
    from jorldy_amd import ops

    rows, inner = [], ops.PPONet.ppo_update_rows
    monkeypatch.setattr(ops.PPONet, "ppo_update_rows", lambda self, x, idx, *a, **kw: (rows.append(int(idx.numel())), inner(self, x, idx, *a, **kw))[1])
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("JH_PPO_ONEPASS", mode)
        agent = Agent("ppo", state_size=S, action_size=A, hidden_size=H, network="continuous_policy_value" if cont else "discrete_policy_value",
                      optim_config={"name": "adam", "lr": lr}, batch_size=2048, n_step=Tn, n_epoch=E, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0,
                      ent_coef=0.01, clip_grad_norm=0.5, gamma=0.99, run_step=100000, num_workers=W, device="cuda", backend="native", use_graph=False)
        assert agent.backend == "native"
        rec = synth.ppo_recipe({k: v.shape for k, v in agent.network.state_dict().items()}, 3)
        agent.network.load_state_dict({k: torch.from_numpy(v) for k, v in rec.items()})
        trs = synth.ppo_rollout(np.random.RandomState(7), M, S, A, bool(cont), clamp_every=0)
        cols = {k: np.concatenate([t[k] for t in trs], 0) for k in ("state", "next_state", "reward", "done", "action")}
        agent.memory.first_store = False
        np.random.seed(5)
        agent.process(cols, Tn)
        torch.cuda.synchronize()
        n_upd = E * 2
        net = agent._net
        out[mode] = {"statistics of every update": npy(agent._stats[:n_upd]).copy(), "weights": npy(net.params).copy(), "exp_avg": npy(net.m).copy(),
                     "exp_avg_sq": npy(net.v).copy(), "last clipped gradient": npy(net.grads).copy()}
        assert np.isfinite(out[mode]["statistics of every update"]).all() and not (out[mode]["statistics of every update"] == -1).all()
    assert rows == [2048, 1042] * E, rows  # (JH_PPO_ONEPASS=1 only: these are the shapes the agent hands to the one call)
    _assert_same_bits(out["1"], out["0"], f"learn() cont={cont}: the one-call update vs the separate calls")
