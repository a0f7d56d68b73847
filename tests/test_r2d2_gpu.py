"""R2D2 on the GPU: the LSTM step kernel and its backward against float64 at rows and widths on both sides of every tile edge, with two row
groups of different weights in one launch; the sequence loss kernel over the sweep of tests/r2d2_truth.py; the network object's three
passes, backpropagation through time and clip + Adam against float64; its acting step; the agent: learn() against the float64 statement
of the reference's learn() on the batch it sampled, graph replay against eager, the acting trace, stored rows, checkpoints."""
import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import r2d2_truth as D
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5


# ---------------------------------------------------------------------------------------------- the step kernel
def _step_case(rows, H, A, seed):
    """One group's inputs in float64, rounded to float32 values: xproj = x W_ih^T + b_ih + b_hh from an input row of H + A entries."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + H + A)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    k = 1.0 / np.sqrt(H)  # torch.nn.LSTM's initial range
    w_ih, w_hh, b = k * r(4 * H, H + A), k * r(4 * H, H), k * r(4 * H)
    xproj = (r(rows, H + A) @ w_ih.t() + b).float().double()
    return dict(xproj=xproj, w_hh=w_hh.float().double(), h=(0.5 * r(rows, H)).float().double(), c=r(rows, H).float().double())


def _against(ours, exact, ref32, what):
    assert torch.isfinite(ours).all(), what
    return T.vs_exact(ours, exact, ref32, TOL, what)


@pytest.mark.parametrize("rows,H,A", D.STEP_SHAPES, ids=[f"R{r}-H{h}-A{a}" for r, h, a in D.STEP_SHAPES])
def test_lstm_step_matches_float64_with_two_row_groups_in_one_launch(rows, H, A):
    """h, c and the four activated gates of both groups (different weights, different row counts) by fp64_truth.vs_exact at TOL against the
    explicit float64 cell, torch-CPU-float32 beside it; then the same launch with the first group empty: the second group's bits do not move."""
    from jorldy_amd import ops

    cases = [_step_case(rows, H, A, 1), _step_case(rows + 3, H, A, 2)]
    # the rows of the first group's xproj sit in a wider buffer: a row stride that is not 4H
    wide = torch.zeros(rows, 4 * H + 8, dtype=torch.float32, device="cuda")
    wide[:, :4 * H] = f32(cases[0]["xproj"])
    xps = [wide[:, :4 * H], f32(cases[1]["xproj"])]
    groups = [(xp, f32(c["w_hh"]), f32(c["h"]), f32(c["c"])) for xp, c in zip(xps, cases)]
    outs = ops.lstm_step(groups, want_gates=True)
    torch.cuda.synchronize()
    for s, (c, out) in enumerate(zip(cases, outs)):
        exact = D.lstm_cell(c["xproj"], c["h"], c["c"], c["w_hh"])
        ref32 = D.lstm_cell(*(c[k].float() for k in ("xproj", "h", "c", "w_hh")))
        for name, o, e, r32 in zip(("h", "c", "gates"), out, exact, ref32):
            _against(o, e, r32, f"R{rows} H{H} group {s} {name}")
    empty = (torch.zeros(0, 4 * H, dtype=torch.float32, device="cuda"), groups[0][1], torch.zeros(0, H, dtype=torch.float32, device="cuda"),
             torch.zeros(0, H, dtype=torch.float32, device="cuda"))
    again = ops.lstm_step([empty, groups[1]], want_gates=True)
    torch.cuda.synchronize()
    assert again[0][0].shape == (0, H)
    for o, e in zip(again[1], outs[1]):
        assert npy(o).tobytes() == npy(e).tobytes(), "one group empty: the other group's result is bit-identical"
    nog = ops.lstm_step(groups[:1])
    assert nog[0][2] is None and npy(nog[0][0]).tobytes() == npy(outs[0][0]).tobytes()


@pytest.mark.parametrize("rows,H,A", D.STEP_SHAPES, ids=[f"R{r}-H{h}-A{a}" for r, h, a in D.STEP_SHAPES])
def test_lstm_step_backward_matches_float64_autograd_over_two_chained_steps(rows, H, A):
    """Two steps t, t + 1 under float64 autograd with loss = <h_{t+1}, G1> + <c_{t+1}, G2> + <h_t, E>.  The kernel runs step t + 1 (dh_ext = G1,
    dc_in = G2, nothing recurrent) and then step t (dh_ext = E, dc_in and dgates_next from the first call): the gradients of both steps'
    pre-activation gates and dc_{t-1} must be autograd's, by fp64_truth.vs_exact at TOL with the float32 autograd beside it."""
    from jorldy_amd import ops

    c0, c1 = _step_case(rows, H, A, 3), _step_case(rows, H, A, 4)
    g = torch.Generator().manual_seed(rows + H)
    G1, G2, E = (torch.randn(rows, H, generator=g, dtype=torch.float64).float().double() for _ in range(3))

    def run(dt):
        xp0, xp1, cprev = (v.to(dt).clone().requires_grad_(True) for v in (c0["xproj"], c1["xproj"], c0["c"]))
        w, h0 = c0["w_hh"].to(dt), c0["h"].to(dt)
        h1, cc1, gates1 = D.lstm_cell(xp0, h0, cprev, w)
        h2, cc2, gates2 = D.lstm_cell(xp1, h1, cc1, w)
        ((h2 * G1.to(dt)).sum() + (cc2 * G2.to(dt)).sum() + (h1 * E.to(dt)).sum()).backward()
        return dict(dg1=xp0.grad, dg2=xp1.grad, dc=cprev.grad, gates1=gates1.detach(), gates2=gates2.detach(), c1=cc1.detach(), c2=cc2.detach())

    t64, t32 = run(torch.float64), run(torch.float32)
    w = f32(c0["w_hh"])
    dg2, dc1 = ops.lstm_step_backward(w, f32(t64["gates2"]), f32(t64["c1"]), f32(t64["c2"]), dh_ext=f32(G1), dc_in=f32(G2))
    dg1, dc0 = ops.lstm_step_backward(w, f32(t64["gates1"]), f32(c0["c"]), f32(t64["c1"]), dh_ext=f32(E), dc_in=dc1, dgates_next=dg2)
    torch.cuda.synchronize()
    _against(dg2, t64["dg2"], t32["dg2"], f"R{rows} H{H} dgates of the last step")
    _against(dg1, t64["dg1"], t32["dg1"], f"R{rows} H{H} dgates of the step before (recurrent product included)")
    _against(dc0, t64["dc"], t32["dc"], f"R{rows} H{H} dc handed to the step before")
    # no gradient from above and none handed down: only the recurrent product feeds the step
    dg1b, _ = ops.lstm_step_backward(w, f32(t64["gates1"]), f32(c0["c"]), f32(t64["c1"]), dgates_next=dg2)
    dg1c, _ = ops.lstm_step_backward(w, f32(t64["gates1"]), f32(c0["c"]), f32(t64["c1"]), dh_ext=torch.zeros_like(dc1), dc_in=torch.zeros_like(dc1), dgates_next=dg2)
    assert npy(dg1b).tobytes() == npy(dg1c).tobytes(), "absent inputs are zeros"


def test_lstm_step_rejects_bad_sizes():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    for H in (6, 2):  # H % 4 != 0, H < 4
        with pytest.raises(JhError):
            ops.lstm_step([(z(3, 4 * H), z(4 * H, H), z(3, H), z(3, H))])
        with pytest.raises(JhError):
            ops.lstm_step_backward(z(4 * H, H), z(3, 4 * H), z(3, H), z(3, H))


# ---------------------------------------------------------------------------------------------- the loss kernel
def _run_loss(c, eta):
    from jorldy_amd import ops

    g, prio, stats, td = ops.r2d2_loss(f32(c["q"]), f32(c["next_q"]), f32(c["next_target_q"]), f32(c["action"]), f32(c["reward"]), f32(c["done"]), f32(c["weights"]),
                                       c["burn"], c["n_step"], D.GAMMA, eta, D.ALPHA, D.EPS, want_td=True)
    torch.cuda.synchronize()
    return npy(g), npy(prio), npy(stats), npy(td)


@pytest.mark.parametrize("B,T_,A", D.SWEEP_SHAPES, ids=[f"B{b}-T{t}-A{a}" for b, t, a in D.SWEEP_SHAPES])
def test_loss_kernel_matches_float64_over_the_sweep(B, T_, A):
    """n_step in {1, 3} x |Q| at 0.05 and 50 x eta in {0, 0.9, 1}: |td|, the float64 priority, the loss, max_Q and d(loss)/dq against the float64
    truth (the reference's rescale expressions as written, in float64) at 1e-5 of the largest entry; the gradient is zero everywhere but at
    the last step's taken action."""
    for n_step, scale, eta in D.SWEEP_VARIANTS:
        c = D.sweep_case(B, T_, A, n_step, scale)
        t = D.sweep_truth(c, eta)
        g, prio, stats, td = _run_loss(c, eta)
        what = f"B{B} T{T_} A{A} n{n_step} |Q|~{scale} eta{eta}"
        assert np.isfinite(g).all() and np.isfinite(prio).all() and np.isfinite(stats).all(), what
        # |td| is a difference of q and the target: its error is measured against the largest of those
        big = max(np.abs(t["target_q"]).max(), np.abs(t["q_taken"]).max())
        margins.leq(np.abs(td - t["td"]).max() / big, TOL, f"{what} |td| / max(|target|, |q|)")
        margins.leq(np.abs(prio - t["priority"]).max() / (big ** D.ALPHA), TOL, f"{what} priority")
        assert prio.dtype == np.float64
        margins.leq(abs(float(stats[0]) - t["loss"]) / (big * big), TOL, f"{what} loss / max^2")
        assert stats[1] == np.float32(t["max_Q"]), "max_Q is an input value: exact"
        assert stats[5] == 0.0 and stats[7] == 0.0
        margins.leq(np.abs(g - t["grad_q"]).max() / (2.0 * big / B), TOL, f"{what} d(loss)/dq / (2 max / B)")
        mask = np.ones_like(g, bool)
        mask[T_ - 1, np.arange(B), np.clip(c["action"][:, c["burn"] + T_ - 1].astype(np.int64), 0, A - 1)] = False
        assert not g[mask].any(), f"{what}: only the last step's taken action has a gradient"


def test_loss_kernel_is_bit_identical_across_runs_and_rejects_bad_sizes():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    c = D.sweep_case(64, 40, 5, 3, 50.0)
    r1, r2 = _run_loss(c, 0.9), _run_loss(c, 0.9)
    for a, b in zip(r1, r2):
        assert a.tobytes() == b.tobytes()
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    # B over the cap, seq_len over 128, A < 2, A over 64, n_step < 1
    for B, T_, A, burn, n in ((1025, 1, 2, 1, 1), (2, 100, 2, 29, 1), (2, 2, 1, 1, 1), (2, 2, 65, 1, 1), (2, 2, 2, 1, 0)):
        cols = max(1, T_ + burn + n - 1)
        with pytest.raises(JhError):
            ops.r2d2_loss(z(T_, B, A), z(T_, B, A), z(T_, B, A), z(B, cols), z(B, cols), z(B, cols), z(B), burn, n, 0.99, 0.9, 0.6)


# ---------------------------------------------------------------------------------------------- the network object
def _mirror64(S, A, H, seed):
    torch.manual_seed(seed)
    m = D.Net(S, A, D_hidden=H).double()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))  # biases away from their zero initialisation
    T.round_to_fp32_(m)
    return m, T.as32(m)


@pytest.mark.parametrize("seq,burn,n,B,H,S,A", D.NET_SHAPES, ids=[f"seq{s[0]}-burn{s[1]}-n{s[2]}-B{s[3]}-H{s[4]}" for s in D.NET_SHAPES])
def test_r2d2net_three_passes_bptt_and_clipped_adam_match_float64(seq, burn, n, B, H, S, A):
    """learn_forward (three passes in lockstep), backward from a gradient on EVERY trained step, and two teacher-forced clip + Adam steps of
    ops.R2D2Net by fp64_truth's criteria: values and raw gradients within max(TOL, 2 x torch-CPU-float32's own error) of float64, the step as
    arithmetic on our own gradient.  The truth runs the burn-in steps without gradient (r2d2_truth.passes), so every gradient below the LSTM
    matching it means the native burn-in steps contribute none either; a row is zero-padded, another ends an episode mid-window."""
    from jorldy_amd import ops
    from test_rbnet_gpu import _force, _grads_vs_exact, _native_state

    ref64, ref32 = _mirror64(S, A, H, 0)
    tgt64, tgt32 = _mirror64(S, A, H, 100)
    nat = ops.R2D2Net(S, A, H, B, seq, burn, n, "cuda:0")
    nat.import_state(ref32.state_dict(), nat.params)
    nat.import_state(tgt32.state_dict(), nat.target)
    sd = nat.export_state()
    assert list(sd.keys()) == list(ref32.state_dict().keys()) and len(sd) == 16
    for k, v in ref32.state_dict().items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), k
    lr, clip = 1e-3, 0.5
    truth = T.OptimTruth(ref64, ref32, lambda ps: torch.optim.Adam(ps, lr=lr), lr, ("exp_avg", "exp_avg_sq"))
    rs = np.random.RandomState(seq + B)
    g = torch.Generator().manual_seed(1)
    tm = lambda v: v.permute(1, 0, 2)  # [B, T', A] -> time-major
    for it in range(2):
        _force(nat, truth, lambda step: nat.set_hyper(lr, 0.9, 0.999, 1e-8, step), it)
        b = D.batch(rs, B, seq, n, S, A, H, pad_rows=(B - 1,) if B > 1 else (), done_rows=(0,))
        out = nat.learn_forward(*(f32(b[k]) for k in ("state", "prev_action_onehot", "hidden_h", "hidden_c", "next_hidden_h", "next_hidden_c")))
        if it == 0:  # an acting step between learn_forward and backward has buffers of its own: the gradients below do not notice it
            nat.act_step(torch.randn(B, S, device="cuda"), torch.zeros(B, A, device="cuda"), torch.randn(B, H, device="cuda"), torch.randn(B, H, device="cuda"))
        truth.opt64.zero_grad()
        truth.opt32.zero_grad()
        q64 = D.passes(ref64, tgt64, b, seq, burn, n)
        q32 = D.passes(ref32, tgt32, b, seq, burn, n)
        for j, name in enumerate(("online over state[:, :seq_len]", "online over state[:, n_step:]", "target over state[:, n_step:]")):
            assert torch.isfinite(out[j]).all()
            T.vs_exact(out[j], tm(q64[j]), tm(q32[j]), TOL, f"step {it} {name}")
        gl = torch.randn(B, seq - burn, A, generator=g) / (B * (seq - burn))
        q64[0].backward(gl.double())
        q32[0].backward(gl)
        nat.backward(tm(gl).contiguous().cuda())
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"step {it} ")
        assert torch.equal(raw["lstm.bias_ih_l0"], raw["lstm.bias_hh_l0"]), "two parameters, one gradient"
        nat.optim_step("adam", clip)
        truth.step(clip, raw, *_native_state(nat), tag=f"clip + adam step {it}")
    with pytest.raises(ValueError):
        nat.optim_step("rmsprop", None)


def test_r2d2net_act_step_carries_the_state_like_the_sequence_forward():
    """Five acting steps of four rows, the carried state handed from one to the next on the device, against the float64 network run over the
    five-step sequence at once: q of every step and the final state."""
    from jorldy_amd import ops

    S, A, H, N, steps = 5, 3, 36, 4, 5
    ref64, ref32 = _mirror64(S, A, H, 3)
    nat = ops.R2D2Net(S, A, H, 8, 4, 1, 2, "cuda:0")
    nat.import_state(ref32.state_dict(), nat.params)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, steps, S, generator=g)
    oh = torch.eye(A)[torch.randint(0, A, (N, steps), generator=g)]
    oh[:, 0] = 0.0  # an episode start: no previous action
    h = c = torch.zeros(N, H, device="cuda")
    qs = []
    for t in range(steps):
        q, h, c = nat.act_step(x[:, t].contiguous().cuda(), oh[:, t].contiguous().cuda(), h, c)
        qs.append(q)
    q64, (h64, c64) = ref64(x.double(), oh.double())
    q32, (h32, c32) = ref32(x, oh)
    T.vs_exact(torch.stack(qs, 1), q64, q32, TOL, "act_step q over five carried steps")
    T.vs_exact(h, h64, h32, TOL, "carried h")
    T.vs_exact(c, c64, c32, TOL, "carried c")


def test_r2d2net_rejects_unsupported_sizes():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    # H % 4, A < 2, A > 64, batch over 1024, seq_len over 128, burn-in not inside the sequence
    for S, A, H, B, seq, burn, n in ((4, 2, 6, 2, 4, 1, 1), (4, 1, 8, 2, 4, 1, 1), (4, 65, 8, 2, 4, 1, 1), (4, 2, 8, 1025, 4, 1, 1), (4, 2, 8, 2, 129, 1, 1), (4, 2, 8, 2, 4, 4, 1)):
        with pytest.raises(JhError):
            ops.R2D2Net(S, A, H, B, seq, burn, n, "cuda:0")


# ---------------------------------------------------------------------------------------------- the agent
CFG = dict(S=4, A=3, H=64, B=8, seq=4, burn=1, n=3)        # the first fixture's shape (padding on)
CFG_ODD = dict(S=5, A=5, H=36, B=7, seq=6, burn=3, n=2)    # odd everything, padding off
CFG_CARTPOLE = dict(S=4, A=2, H=512, B=64, seq=4, burn=1, n=3, steps=200)  # config.r2d2.cartpole's network and batch


def _agent(cfg, use_graph=True, zero_padding=True, seed=0, **over):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(seed)
    np.random.seed(seed)
    kw = dict(state_size=cfg["S"], action_size=cfg["A"], hidden_size=cfg["H"], network="r2d2", head="mlp", optim_config={"name": "adam", "lr": 1e-3},
              batch_size=cfg["B"], n_step=cfg["n"], seq_len=cfg["seq"], n_burn_in=cfg["burn"], zero_padding=zero_padding, buffer_size=64, start_train_step=0,
              run_step=1000, lr_decay=False, clip_grad_norm=40.0, use_graph=use_graph, epsilon=0.4, gamma=0.99, eta=0.9, alpha=0.6, beta=0.4)
    kw.update(over)
    return Agent("r2d2", **kw)


def _interact(agent, cfg, steps, seed=1, episode=11, store=True):
    """The reference's single-actor loop on synthetic states with an episode end every `episode` steps: act -> interact_callback -> store.
    -> (acting outputs per step, emitted rows)."""
    rs = np.random.RandomState(seed)
    state, trace, rows = rs.randn(1, cfg["S"]).astype(np.float32), [], []
    for t in range(steps):
        out = agent.act(state)
        nxt = rs.randn(1, cfg["S"]).astype(np.float32)
        done = (t + 1) % episode == 0
        tr = {"state": state, "next_state": nxt, "reward": np.asarray([[rs.choice([-1.0, 0.0, 1.0, 0.5])]], np.float32), "done": np.asarray([[done]])}
        tr.update(out)
        trace.append(dict(out, done=done, state=state))
        row = agent.interact_callback(tr)
        if row:
            rows.append(row)
            if store:
                agent.memory.store([row])
        state = nxt
    return trace, rows


def _truth_nets(agent, cfg):
    nets = []
    for view in (agent.network, agent.target_network):
        m = D.Net(cfg["S"], cfg["A"], D_hidden=cfg["H"]).double()
        m.load_state_dict({k: v.double().cpu() for k, v in view.state_dict().items()})
        nets.append(m)
    return nets


@pytest.mark.parametrize("cfg,pad", ((CFG, True), (CFG_ODD, False), (CFG_CARTPOLE, True)), ids=("padded", "odd", "cartpole"))
def test_agent_learn_is_the_float64_learn_on_the_batch_it_sampled(cfg, pad):
    """Buffer filled by the agent's own act / interact_callback loop (episode ends, zero-padded rows where padding is on), then two eager
    learns.  Each is held to r2d2_truth.learn in float64 from the weights the agent had and the batch it sampled: loss, max_Q, the tree
    leaves after the write-back (float64 priorities), and the step as arithmetic on our own clipped gradient."""
    agent = _agent(cfg, use_graph=False, zero_padding=pad)
    _interact(agent, cfg, cfg.get("steps", 60 if pad else 160), episode=11 if pad else 23)  # (without padding only full windows are stored: longer episodes)
    assert agent.memory.size >= cfg["B"]
    np.random.seed(5)
    beta0 = agent.beta
    for k in range(2):
        ref64, tgt64 = _truth_nets(agent, cfg)
        w0 = {k_: v.clone() for k_, v in agent.network.state_dict().items()}
        r = agent.learn()
        st = agent._static
        b = {k_: npy(v) for k_, v in st["tr"].items()}
        if pad:
            assert any(not b["state"][i, 0].any() for i in range(cfg["B"])) or k > 0, "the first batch holds a zero-padded row"
        t = D.learn(ref64, tgt64, b, npy(st["w"]), cfg["seq"], cfg["burn"], cfg["n"], np.float32(0.99), np.float32(0.9), np.float32(0.6))
        big = float(t["target_q"].abs().max())
        margins.leq(abs(r["loss"] - t["loss"]) / big ** 2, TOL, f"learn {k} loss / max target^2")
        margins.leq(abs(r["max_Q"] - t["max_Q"]) / big, TOL, f"learn {k} max_Q")
        leaves = agent.memory.sum_tree[npy(st["idx"])]
        margins.leq(np.abs(leaves - t["priority"][:, 0].numpy()).max() / big ** 0.6, TOL, f"learn {k} tree leaves after the write-back")
        g = agent._net.export_state(agent._net.grads)
        w1 = agent.network.state_dict()
        T.check_first_step_from_our_gradient(w0, g, w1, lambda ps: torch.optim.Adam(ps, lr=1e-3), 1e-3, f"learn {k}") if k == 0 else None
        assert r["num_learn"] == k + 1 and set(r) == {"loss", "max_Q", "sampled_p", "mean_p", "num_learn", "num_transitions"}
    assert agent.beta == min(1.0, beta0 + 2 * agent.beta_add), "beta is annealed once per learn()"


def test_agent_graph_replay_equals_eager_bit_for_bit():
    """Two agents from one seed and one buffer history: four learns eagerly, four with the hipGraph (warm eager call, capture, replays).  Losses,
    weights, moments and the sum tree must be identical bits."""
    out = []
    for use_graph in (False, True):
        agent = _agent(CFG, use_graph=use_graph)
        _interact(agent, CFG, 60)
        np.random.seed(9)
        res = [agent.learn() for _ in range(4)]
        torch.cuda.synchronize()
        out.append((res, {k: npy(v) for k, v in agent.network.state_dict().items()}, npy(agent._net.m), npy(agent._net.v), agent.memory.sum_tree.copy()))
    (r0, w0, m0, v0, t0), (r1, w1, m1, v1, t1) = out
    for a, b in zip(r0, r1):
        assert a == b
    for k in w0:
        assert w0[k].tobytes() == w1[k].tobytes(), k
    assert m0.tobytes() == m1.tobytes() and v0.tobytes() == v1.tobytes() and t0.tobytes() == t1.tobytes()


def test_agent_acting_trace_carries_and_resets_the_state_in_the_references_draw_order():
    """Across an episode end: q and the greedy action against the float64 network stepped with the same carried state; hidden_h / hidden_c are the
    state going IN; zeros and a zero one-hot after `done`; np.random.random() is drawn before randint, and randint only when exploring."""
    agent = _agent(CFG, epsilon=0.5)
    ref64, _ = _truth_nets(agent, CFG)
    np.random.seed(3)
    st0 = np.random.get_state()
    trace, _ = _interact(agent, CFG, 14, episode=6, store=False)
    np.random.set_state(st0)
    h = c = torch.zeros(1, CFG["H"], dtype=torch.float64)
    prev = None
    for t, o in enumerate(trace):
        oh = np.zeros((1, CFG["A"]), np.float32) if prev is None else np.eye(CFG["A"], dtype=np.float32)[prev.reshape(-1)]
        assert np.array_equal(o["prev_action_onehot"], oh), t
        margins.leq(np.abs(o["hidden_h"][0] - h.numpy()).max(), 1e-5, f"step {t} hidden_h going in")
        margins.leq(np.abs(o["hidden_c"][0] - c.numpy()).max(), 1e-5, f"step {t} hidden_c going in")
        assert o["hidden_h"].shape == (1, 1, CFG["H"]) and o["q"].shape == (1, 1) and o["action"].shape == (1, 1)
        q, (h, c) = ref64(torch.as_tensor(o["state"]).double()[:, None], torch.as_tensor(oh).double()[:, None], (h, c))
        q = q[0, 0].detach().numpy()
        h, c = h.detach(), c.detach()
        explore = np.random.random() < 0.5
        want = np.random.randint(0, CFG["A"], size=(1, 1)) if explore else np.asarray([[int(q.argmax())]])
        assert np.array_equal(o["action"], want), (t, explore)
        margins.leq(abs(float(o["q"][0, 0]) - q[want[0, 0]]), 1e-5 * max(1.0, np.abs(q).max()), f"step {t} q of the action taken")
        prev = o["action"]
        if o["done"]:
            h = c = torch.zeros(1, CFG["H"], dtype=torch.float64)
            prev = None
    assert sum(o["done"] for o in trace) == 2


def test_agent_act_returns_each_rows_own_q():
    agent = _agent(CFG, epsilon=0.0)
    out = agent.act(np.random.RandomState(0).randn(5, CFG["S"]).astype(np.float32))
    q, _, _ = agent.network(torch.as_tensor(np.random.RandomState(0).randn(5, 1, CFG["S"]).astype(np.float32)), torch.zeros(5, 1, CFG["A"]))
    q = npy(q)[:, 0]
    assert out["action"].shape == (5, 1) and np.array_equal(out["action"][:, 0], q.argmax(-1)) and np.array_equal(out["q"][:, 0], q.max(-1))


@pytest.mark.parametrize("pad", (True, False))
def test_interact_callback_emits_windows_with_actor_priorities(pad):
    """Rows come every seq_len // 2 steps and at once after an episode start; shapes are those of a seq_len + n_step window; with padding the short
    windows are left-padded with zeros (float64, action included); the priority is the sequence priority of the actor's own q values."""
    cfg = CFG_ODD
    agent = _agent(cfg, zero_padding=pad)
    trace, rows = _interact(agent, cfg, 40, episode=13)
    L = cfg["seq"] + cfg["n"]
    assert rows
    for r in rows:
        assert r["state"].shape == (1, L, cfg["S"]) and r["prev_action_onehot"].shape == (1, L, cfg["A"])
        for k in ("action", "reward", "done"):
            assert r[k].shape == (1, L - 1, 1), k
        for k in ("hidden_h", "hidden_c", "next_hidden_h", "next_hidden_c"):
            assert r[k].shape == (1, 1, cfg["H"]), k
        assert r["priority"].shape == (1, 1) and np.isfinite(r["priority"]).all() and "q" not in r
    padded = [r for r in rows if r["action"].dtype == np.float64]
    assert bool(padded) == pad
    for r in padded:
        assert not r["state"][0, 0].any() and not r["prev_action_onehot"][0, 0].any()
    assert agent.memory.size == len(rows)
    tree = agent.memory.sum_tree[agent.memory.first_leaf_index:agent.memory.first_leaf_index + len(rows)]
    np.testing.assert_allclose(tree, [float(r["priority"].reshape(-1)[0]) for r in rows], rtol=1e-12)


def test_agent_checkpoint_round_trip_and_optimizer_state_loads_into_torch_adam(tmp_path):
    agent = _agent(CFG)
    _interact(agent, CFG, 40)
    np.random.seed(2)
    for _ in range(3):
        agent.learn()
    agent.save(str(tmp_path))
    ck = torch.load(str(tmp_path / "ckpt"), map_location="cpu", weights_only=False)
    assert set(ck) == {"network", "optimizer"} and len(ck["network"]) == 16
    params = [torch.nn.Parameter(v.clone()) for v in ck["network"].values()]
    opt = torch.optim.Adam(params, lr=1e-3)
    opt.load_state_dict(ck["optimizer"])
    assert float(opt.state[params[0]]["step"]) == 3.0 and opt.state[params[2]]["exp_avg"].shape == params[2].shape
    other = _agent(CFG, seed=7)
    other.load(str(tmp_path))
    for k, v in agent.network.state_dict().items():
        assert torch.equal(v, other.network.state_dict()[k]), k
    assert torch.equal(agent._net.m, other._net.m) and torch.equal(agent._net.v, other._net.v) and other._adam_steps == 3


def test_unsupported_configurations_raise_at_construction():
    base = dict(state_size=4, action_size=2, hidden_size=64, batch_size=8, seq_len=4, n_burn_in=1, n_step=2)
    from jorldy_amd.core.agent import Agent

    for bad in (dict(head="cnn", state_size=(4, 84, 84)), dict(state_size=(4, 4)), dict(hidden_size=66), dict(action_size=1), dict(action_size=65), dict(seq_len=129, n_burn_in=40),
                dict(batch_size=1025), dict(optim_config={"name": "rmsprop"}), dict(frame_dedup=True), dict(grad_sync=object()), dict(n_burn_in=4)):
        with pytest.raises(ValueError, match="R2D2 runs on libjorldy_hip only"):
            Agent("r2d2", **dict(base, **bad))


# ---------------------------------------------------------------------------------------------- against the reference's recorded output
def _rel(a, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64).reshape(ref.shape) - ref).max() / (np.abs(ref).max() + 1e-30))


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_acts_stores_and_learns_like_the_reference_fixture(name):
    """tools/gen_golden_r2d2.py's run of the unmodified reference, repeated with the native agent from the same starting weights, states and seeds:
      initial weights   a fresh agent under the fixture's torch seed has the reference's initialisation (to H x 2^-23: orthogonal_'s float32 QR)
      acting trace      across an episode end: the same actions and one-hots (dtype included), q and the carried state going in at 1e-5
      stored rows       as many, padded where the reference padded (float64 columns), every column at 1e-5 of its largest entry (the exact
                        ones exactly), the actor priorities and the tree after the fill at 1e-5
      two learns        the reference's sampled indices (both samples); q_pred and both next-Q tensors; loss and max_Q; the priorities
                        written back (every leaf, compared before the power alpha); p.grad as the optimizer sees it, Adam's moments and the
                        weights with the caps of test_iqn_agent_learn_matches_reference; beta.  Target-dependent quantities of r2d2_cartpole
                        at 2 x hyper/ref_target_err + 1e-5 = 8.9e-5, everything else at 1e-5.  In the second learn the online network's
                        forwards and the IS weights are target-dependent too (the first learn's gradient and write-back).  Measured: every
                        forward of both learns of r2d2 / r2d2_odd within 4.6e-7 of the largest entry; r2d2_cartpole 6.3e-7 in the first
                        learn, 1.3e-5 (online) and 5.2e-7 (target network) in the second, its second IS weights 1.3e-5."""
    from jorldy_amd.core.agent import Agent

    f = D.Fixture(name)
    z = f.z
    torch.manual_seed(f.init_seed)
    fresh = Agent("r2d2", **f.agent_kwargs())
    for k, v in fresh.network.state_dict().items():
        # orthogonal_ goes through a float32 Householder QR whose rounding depends on the host's LAPACK blocking: its backward error is
        # n x 2^-24 per reflection pair, n = the layer's width, so two hosts agree to about n x 2^-23 of the largest entry, not bitwise
        margins.leq(_rel(f.thin(npy(v)), z["init_thin/" + k]) if np.abs(z["init_thin/" + k]).max() > 0 else float(np.abs(npy(v)).max()), f.H * 2.0 ** -23, f"{name} initial {k}")
    agent = Agent("r2d2", **f.agent_kwargs(use_graph=False))
    agent.network.load_state_dict(f.weights(0))
    agent.target_network.load_state_dict(f.weights(1))
    trace, rows = D.fill_loop(agent, f)
    # ---- the acting trace
    for t in range(f.trace):
        o = trace[t]
        assert np.array_equal(o["action"], z["trace/action"][t]), f"step {t} action"
        assert np.array_equal(o["prev_action_onehot"], z["trace/prev_action_onehot"][t]) and bool(o["done"]) == bool(z["trace/done"][t])
        assert o["prev_action_onehot"].dtype == (np.float32 if (t == 0 or z["trace/done"][t - 1]) else np.int64), f"step {t}: the one-hot's dtype"
        for k in ("q", "hidden_h", "hidden_c"):
            assert o[k].shape == z["trace/" + k][t].shape, k
            margins.leq(np.abs(o[k] - z["trace/" + k][t]).max(), 1e-5 * max(1.0, np.abs(z["trace/" + k]).max()), f"{name} step {t} {k}")
    # ---- the stored rows and their priorities
    assert len(rows) == f.n_rows and np.array_equal([int(np.asarray(r["action"]).dtype == np.float64) for r in rows], z["rows/padded"])
    for k in D.ROW_KEYS:
        got = f.thin(np.concatenate([np.asarray(r[k]).astype(np.float32) for r in rows], 0))
        if k in ("state", "reward", "done", "action", "prev_action_onehot"):
            assert np.array_equal(got, z["rows/" + k]), k
        else:
            margins.leq(_rel(got, z["rows/" + k]), 1e-5, f"{name} rows {k}")
    prio = np.concatenate([np.asarray(r["priority"], np.float64).reshape(-1) for r in rows])
    margins.leq(_rel(prio, z["rows/priority64"]), 1e-5, f"{name} actor priorities")
    margins.leq(_rel(agent.memory.sum_tree, z["tree0"]), 1e-5, f"{name} tree after the fill")
    # ---- two consecutive learns
    np.random.seed(f.np_seed)
    first_leaf = agent.memory.first_leaf_index
    for k in range(2):
        rec = f.learn(k)
        r = agent.learn()
        st = agent._static
        assert np.array_equal(npy(st["idx"]), rec["learn/indices"]), f"learn {k}: the sampled indices"
        # What the first learn's target reaches in the second: the online weights (through the gradient), the written-back priorities and so the
        # IS weights.  Those are held to the fixture's target tolerance (1e-5; r2d2_cartpole 2 x ref_target_err + 1e-5), everything else to 1e-5.
        tt = f.target_tol
        on_tol = 1e-5 if k == 0 else tt
        margins.leq(_rel(npy(st["w"]), rec["learn/weights"]), on_tol, f"{name} learn {k} IS weights")
        q3 = npy(st["q"]).transpose(0, 2, 1, 3)
        for j_, (key, tol) in enumerate((("q_pred", on_tol), ("next_q", on_tol), ("next_target_q", 1e-5))):
            print(f"{name} learn {k} {key}: {_rel(q3[j_], rec['learn/' + key]):.3e} of the largest entry (cap {tol:.1e})")
            margins.leq(_rel(q3[j_], rec["learn/" + key]), tol, f"{name} learn {k} {key}")
        fwd_tol = on_tol
        big = float(np.abs(rec["learn/target_q"]).max())
        margins.leq(abs(r["loss"] - float(rec["result/loss"])), 2.0 * tt * big * float(np.abs(rec["learn/td_error"]).max()) + 1e-5 * float(rec["result/loss"]), f"{name} learn {k} loss")
        margins.leq(abs(r["max_Q"] - float(rec["result/max_Q"])), fwd_tol * abs(float(rec["result/max_Q"])), f"{name} learn {k} max_Q")
        assert r["num_learn"] == k + 1 and agent.beta == float(rec["beta_after"])
        inv = 1.0 / f.alpha
        leaves, ref_leaves = agent.memory.sum_tree[first_leaf:first_leaf + f.n_rows], rec["tree"][first_leaf:first_leaf + f.n_rows]
        margins.leq(np.abs(leaves ** inv - ref_leaves ** inv).max(), tt * big, f"{name} learn {k} priorities in the tree (before the power alpha) / max |target|")
        margins.leq(_rel(agent.memory.sum_tree[0], rec["tree"][0]), 10 * tt, f"{name} learn {k} root of the tree")
        gtol = tt
        grads = {kk: npy(v) for kk, v in agent._net.export_state(agent._net.grads).items()}
        for kk, g in grads.items():
            margins.leq(np.abs(f.thin(g) - rec["grad_thin/" + kk]).max(), gtol * float(rec["grad_absmax/" + kk]) + 1e-12, f"{name} learn {k} d(loss)/d {kk} / its largest entry")
        for bucket, nm in ((agent._net.m, "exp_avg"), (agent._net.v, "exp_avg_sq")):
            for kk, v in agent._net.export_state(bucket).items():
                margins.leq(_rel(f.thin(npy(v)), rec[f"opt1_thin/{nm}/{kk}"]), 2.0 * max(gtol, 1e-5), f"{name} learn {k} {nm} {kk}")
        tot = bad = 0
        worst = 0.0
        for kk, v in agent.network.state_dict().items():
            dd = np.abs(f.thin(npy(v)) - rec["sd1_thin/" + kk])
            tot += dd.size
            bad += int((dd > 2e-5).sum())
            worst = max(worst, float(dd.max()))
        margins.leq(bad / tot, 0.005, f"{name} learn {k}: fraction of weights further than 2e-5 from the reference's")
        margins.leq(worst, 2.1 * f.lr * (k + 1), f"{name} learn {k}: worst weight difference vs the possible travel")
