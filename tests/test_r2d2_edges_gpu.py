"""R2D2's three kernels at their own dispatch limits (tests/r2d2_truth.py's EDGE tables), against float64 on the CPU:
  jh_lstm_step            four row groups in one launch with the empty one in the middle, at every split of the k chunks over the four
                          waves, partial unit tiles and k chunks, rows on both sides of the 16-row tile; each group bit-identical to the same
                          group launched alone
  jh_lstm_step_backward   the same shapes through two chained steps of float64 autograd
  jh_r2d2_loss            up to its cap of 1024 rows (16 waves), A = 64, T' + burn-in = 128, n_step > T' and n_step = 128, with variants that
                          need no tolerance: max_Q found in any wave, the loss delivered from any wave, the action clamp, exact ties
  R2D2Net                 two row tiles with a partial unit tile at every step launch; a batch smaller than max_batch, then the full one
Tolerances and criteria are those of tests/test_r2d2_gpu.py; that the inputs would expose a lost wave, k chunk or unit tile is shown without
a GPU in tests/test_r2d2_cpu.py."""
import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import r2d2_truth as D
import test_r2d2_gpu as G
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

TOL = G.TOL
STEP_IDS = [f"R{r}-H{h}-A{a}" for r, h, a in D.EDGE_STEP_SHAPES]


def _same_bits(a, b, what):
    assert npy(a).tobytes() == npy(b).tobytes(), what


# ---------------------------------------------------------------------------------------------- the step kernel
@pytest.mark.parametrize("rows,H,A", D.EDGE_STEP_SHAPES, ids=STEP_IDS)
def test_lstm_step_four_groups_match_float64_and_each_equals_itself_alone(rows, H, A):
    """Groups of rows, 0, rows + 3 and 1 rows with weights of their own in one launch, the xproj rows of all but the second inside wider buffers:
    h, c and the gates of every non-empty group by fp64_truth.vs_exact at TOL against the float64 cell.  A workgroup's arithmetic depends on
    nothing outside its segment, so every group's result has the bits of that group launched alone; a second launch repeats the bits; without
    the gates h and c keep theirs."""
    from jorldy_amd import ops

    cases = D.edge_step_groups(rows, H, A)
    groups = []
    for s, c in enumerate(cases):
        n = c["xproj"].shape[0]
        # a row stride that is not 4H (a single row has no stride to speak of); the empty group as test_r2d2_gpu.py makes it
        wide = torch.zeros(n, 4 * H + (4 * (s + 1) if n else 0), dtype=torch.float32, device="cuda")
        if n:
            wide[:, :4 * H] = f32(c["xproj"])
        h0, c0 = (f32(c[k]) if n else torch.zeros(0, H, dtype=torch.float32, device="cuda") for k in ("h", "c"))
        groups.append((wide[:, :4 * H], f32(c["w_hh"]), h0, c0))
    outs = ops.lstm_step(groups, want_gates=True)
    torch.cuda.synchronize()
    assert [tuple(o[0].shape) for o in outs] == [(rows, H), (0, H), (rows + 3, H), (1, H)]
    live, names = (0, 2, 3), ("h", "c", "gates")
    for s in live:
        c = cases[s]
        exact = D.lstm_cell(c["xproj"], c["h"], c["c"], c["w_hh"])
        ref32 = D.lstm_cell(*(c[k].float() for k in ("xproj", "h", "c", "w_hh")))
        for name, o, e, r32 in zip(names, outs[s], exact, ref32):
            G._against(o, e, r32, f"R{rows} H{H} group {s} of four {name}")
    again, plain = ops.lstm_step(groups, want_gates=True), ops.lstm_step(groups)
    torch.cuda.synchronize()
    for s in live:
        alone = ops.lstm_step([groups[s]], want_gates=True)[0]
        torch.cuda.synchronize()
        for name, o, a, b in zip(names, outs[s], alone, again[s]):
            _same_bits(o, a, f"group {s} {name}: among four groups and alone")
            _same_bits(o, b, f"group {s} {name}: two identical launches")
        assert plain[s][2] is None
        _same_bits(plain[s][0], outs[s][0], f"group {s} h without the gates")
        _same_bits(plain[s][1], outs[s][1], f"group {s} c without the gates")


@pytest.mark.parametrize("rows,H,A", D.EDGE_STEP_SHAPES, ids=STEP_IDS)
def test_lstm_step_backward_matches_float64_autograd_at_the_edge_shapes(rows, H, A):
    """The body of the two-chained-steps test (dgates of both steps and dc_prev by vs_exact at TOL, absent inputs are zeros) at EDGE_STEP_SHAPES:
    K = 4H in H / 4 chunks over the four waves, 2 to 25 and 256 of them."""
    G.test_lstm_step_backward_matches_float64_autograd_over_two_chained_steps(rows, H, A)


@pytest.mark.parametrize("rows,H", ((33, 68), (17, 1024)))
def test_lstm_step_backward_is_bit_identical_across_runs(rows, H):
    from jorldy_amd import ops

    g = torch.Generator().manual_seed(H)
    n = lambda *s: torch.randn(*s, generator=g).cuda()
    w, gates = n(4 * H, H) / np.sqrt(H), torch.rand(rows, 4 * H, generator=g).cuda()
    c_prev, c, dh, dc, dgn = n(rows, H), n(rows, H), n(rows, H), n(rows, H), n(rows, 4 * H)
    runs = [ops.lstm_step_backward(w, gates, c_prev, c, dh_ext=dh, dc_in=dc, dgates_next=dgn) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    _same_bits(runs[0][0], runs[1][0], "dgates")
    _same_bits(runs[0][1], runs[1][1], "dc_prev")


# ---------------------------------------------------------------------------------------------- the loss kernel
def _check_loss(c, eta, what):
    """test_loss_kernel_matches_float64_over_the_sweep's criteria on one case -> (truth, (g_q, priority, stats, td))."""
    B, T_ = c["B"], c["T"]
    t = D.sweep_truth(c, eta)
    g, prio, stats, td = G._run_loss(c, eta)
    assert np.isfinite(g).all() and np.isfinite(prio).all() and np.isfinite(stats).all() and np.isfinite(td).all(), what
    big = max(np.abs(t["target_q"]).max(), np.abs(t["q_taken"]).max())
    margins.leq(np.abs(td - t["td"]).max() / big, TOL, f"{what} |td| / max(|target|, |q|)")
    margins.leq(np.abs(prio - t["priority"]).max() / (big ** D.ALPHA), TOL, f"{what} priority")
    assert prio.dtype == np.float64
    margins.leq(abs(float(stats[0]) - t["loss"]) / (big * big), TOL, f"{what} loss / max^2")
    assert stats[1] == np.float32(t["max_Q"]), f"{what}: max_Q is an input value: exact"
    assert stats[5] == 0.0 and stats[7] == 0.0
    margins.leq(np.abs(g - t["grad_q"]).max() / (2.0 * big / B), TOL, f"{what} d(loss)/dq / (2 max / B)")
    mask = np.ones_like(g, bool)
    mask[T_ - 1, np.arange(B), D.taken(c)[:, -1]] = False
    assert not g[mask].any(), f"{what}: only the last step's taken action has a gradient"
    return t, (g, prio, stats, td)


@pytest.mark.parametrize("B,T_,A,n_step,seed", D.EDGE_LOSS_CASES, ids=[f"B{c[0]}-T{c[1]}-A{c[2]}-n{c[3]}" for c in D.EDGE_LOSS_CASES])
def test_loss_kernel_matches_float64_at_its_limits(B, T_, A, n_step, seed):
    """|Q| at 0.05 and 50, eta 0.9 (EDGE_MULTI also at 0 and 1): the sweep's criteria with 2 to 16 waves, the argmax walk and the g_q zeroing at
    A = 64, T' + burn-in = 128, a fold longer than the trained window."""
    etas = (0.0, D.EDGE_ETA, 1.0) if (B, T_, A, n_step, seed) == D.EDGE_MULTI else (D.EDGE_ETA,)
    for scale in D.EDGE_SCALES:
        c = D.sweep_case(B, T_, A, n_step, scale, seed)
        for eta in etas:
            _check_loss(c, eta, f"B{B} T{T_} A{A} n{n_step} |Q|~{scale} eta{eta}")


@pytest.mark.parametrize("scale", D.EDGE_SCALES)
def test_loss_kernel_variants_that_need_no_tolerance(scale):
    """EDGE_MULTI (16 waves) doctored one property at a time (r2d2_truth.edge_multi_variants), each under the sweep's criteria and then:
      max_Q in row B - 1, in the first row of wave 7, in row 0   stats[1] is exactly that value: thread 0's fold over the waves
      the only non-zero weight in wave 15, in wave 9             the loss is that row's term (the cross-wave half of the block sum) and
                                                                 every other row's g_q is exactly zero
      actions -1, A, A + 3                                       the gradient sits in column 0, A - 1, A - 1
      exact ties of the two best next_q entries                  the first maximum's target (the other one is 2 max|next_target_q| away)
      a row with done = 1 at every column                        its targets are the rescaled rewards."""
    B, T_, A = D.EDGE_MULTI[:3]
    for name, c, info in D.edge_multi_variants(scale):
        what = f"|Q|~{scale} {name}"
        t, (g, prio, stats, td) = _check_loss(c, D.EDGE_ETA, what)
        if "max_q" in info:
            assert stats[1] == info["max_q"] and stats[1].dtype == np.float32, what
        if "only_row" in info:
            others = np.arange(B) != info["only_row"]
            assert (g[:, others, :] == 0.0).all() and np.count_nonzero(g) == 1 and float(stats[0]) > 0.0, what
        if "columns" in info:
            for row, col in info["columns"].items():
                assert g[T_ - 1, row, col] != 0.0 and np.count_nonzero(g[:, row, :]) == 1, f"{what}: row {row} lands on column {col}"


def test_loss_kernel_at_the_cap_repeats_its_bits_with_and_without_td():
    from jorldy_amd import ops

    B, T_, A, n_step, seed = D.EDGE_MULTI
    c = D.sweep_case(B, T_, A, n_step, 50.0, seed)
    r1, r2 = G._run_loss(c, D.EDGE_ETA), G._run_loss(c, D.EDGE_ETA)
    for a, b in zip(r1, r2):
        assert a.tobytes() == b.tobytes(), "two runs at B = 1024"
    g, prio, stats, td = ops.r2d2_loss(f32(c["q"]), f32(c["next_q"]), f32(c["next_target_q"]), f32(c["action"]), f32(c["reward"]), f32(c["done"]), f32(c["weights"]),
                                       c["burn"], c["n_step"], D.GAMMA, D.EDGE_ETA, D.ALPHA, D.EPS, want_td=False)
    torch.cuda.synchronize()
    assert td is None
    for a, b in zip((g, prio, stats), r1):
        assert npy(a).tobytes() == b.tobytes(), "want_td=False: the same bits"


# ---------------------------------------------------------------------------------------------- the network object
def test_r2d2net_three_passes_with_a_second_row_tile_and_a_partial_unit_tile():
    """The body of test_r2d2net_three_passes_bptt_and_clipped_adam_match_float64 at EDGE_NET_SHAPE: B = 17 rows per segment (two row tiles, one
    row in the second), H = 20 (a partial unit tile and a partial k chunk) in every three-segment step launch and every backward step."""
    G.test_r2d2net_three_passes_bptt_and_clipped_adam_match_float64(*D.EDGE_NET_SHAPE)


def test_r2d2net_a_batch_below_max_batch_then_the_full_one():
    """learn_forward strides every buffer by the B it is given: B = 5 on an object made for 17, then 17 on the same object.  Each time the three
    q tensors by vs_exact against r2d2_truth.passes and the raw gradients by test_rbnet_gpu._grads_vs_exact; nothing stale from the smaller
    call may reach the larger one."""
    from jorldy_amd import ops
    from test_rbnet_gpu import _grads_vs_exact

    seq, burn, n, max_b, H, S, A = D.EDGE_NET_SHAPE
    (ref64, ref32), (tgt64, tgt32) = G._mirror64(S, A, H, 0), G._mirror64(S, A, H, 100)
    nat = ops.R2D2Net(S, A, H, max_b, seq, burn, n, "cuda:0")
    nat.import_state(ref32.state_dict(), nat.params)
    nat.import_state(tgt32.state_dict(), nat.target)
    rs = np.random.RandomState(max_b)
    g = torch.Generator().manual_seed(3)
    tm = lambda v: v.permute(1, 0, 2)
    for B in (5, max_b):
        b = D.batch(rs, B, seq, n, S, A, H, pad_rows=(B - 1,), done_rows=(0,))
        out = nat.learn_forward(*(f32(b[k]) for k in ("state", "prev_action_onehot", "hidden_h", "hidden_c", "next_hidden_h", "next_hidden_c")))
        assert tuple(out.shape) == (3, seq - burn, B, A)
        for m in (ref64, ref32):
            for p in m.parameters():
                p.grad = None
        q64 = D.passes(ref64, tgt64, b, seq, burn, n)
        q32 = D.passes(ref32, tgt32, b, seq, burn, n)
        for j, name in enumerate(("online over state[:, :seq_len]", "online over state[:, n_step:]", "target over state[:, n_step:]")):
            assert torch.isfinite(out[j]).all()
            T.vs_exact(out[j], tm(q64[j]), tm(q32[j]), TOL, f"B {B} of max_batch {max_b} {name}")
        gl = torch.randn(B, seq - burn, A, generator=g) / (B * (seq - burn))
        q64[0].backward(gl.double())
        q32[0].backward(gl)
        nat.backward(tm(gl).contiguous().cuda())
        raw = _grads_vs_exact(nat, ref64, ref32, tag=f"B {B} of max_batch {max_b} ")
        assert torch.equal(raw["lstm.bias_ih_l0"], raw["lstm.bias_hh_l0"])
