"""R2D2 without a GPU: the parameter container against the reference's state_dict layout, the float64 truth's recurrence against
torch.nn.LSTM, the kernel tests' sweep kept off every discontinuity of the loss, and the float64 truth against what the unmodified reference
recorded (tools/gen_golden_r2d2.py's fixtures)."""
import copy

import numpy as np
import pytest
import torch

import r2d2_truth as D


def test_network_container_has_the_references_16_keys_shapes_and_initialisation():
    from jorldy_amd.core.agent import R2D2 as R2D2Agent
    from jorldy_amd.core.agent import ApeX, agent_dict
    from jorldy_amd.core.network import R2D2, Network, network_dict

    assert network_dict["r2d2"] is R2D2 and agent_dict["r2d2"] is R2D2Agent and issubclass(R2D2Agent, ApeX)
    S, A, H = 5, 3, 8
    torch.manual_seed(3)
    net = Network("r2d2", S, A, D_hidden=H, head="mlp")
    want = [("head.l.weight", (H, S)), ("head.l.bias", (H,)), ("lstm.weight_ih_l0", (4 * H, H + A)), ("lstm.weight_hh_l0", (4 * H, H)), ("lstm.bias_ih_l0", (4 * H,)),
            ("lstm.bias_hh_l0", (4 * H,)), ("l.weight", (H, H)), ("l.bias", (H,)), ("l1_a.weight", (H, H)), ("l1_a.bias", (H,)), ("l1_v.weight", (H, H)),
            ("l1_v.bias", (H,)), ("l2_a.weight", (A, H)), ("l2_a.bias", (A,)), ("l2_v.weight", (1, H)), ("l2_v.bias", (1,))]
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == want
    # orthogonal_init on the four stream layers (zero biases, orthogonal rows or columns) and on the head; the LSTM and `l` keep torch's defaults
    for name in ("l1_a", "l1_v", "l2_a", "l2_v"):
        assert not getattr(net, name).bias.detach().any()
    w = net.l1_a.weight.detach().double()
    assert torch.allclose(w @ w.t(), 2.0 * torch.eye(H, dtype=torch.float64), atol=1e-5)  # gain sqrt(2)
    w = net.l2_a.weight.detach().double()
    assert torch.allclose(w @ w.t(), torch.eye(A, dtype=torch.float64), atol=1e-5)
    assert net.l.bias.detach().any() and net.lstm.bias_ih_l0.detach().any() and net.lstm.bias_hh_l0.detach().any()
    assert float(net.lstm.weight_hh_l0.detach().abs().max()) <= 1.0 / np.sqrt(H)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 1, S), torch.zeros(1, 1, A))  # a parameter container: the product computes natively


@pytest.mark.parametrize("B,T,S,A,H", ((1, 1, 3, 2, 4), (3, 7, 5, 5, 36)))
def test_truth_recurrence_is_torch_lstm_forward_and_gradients(B, T, S, A, H):
    """The explicit equations of r2d2_truth.Net.recur against torch.nn.LSTM(...).double() on the same parameters: outputs, final state and every
    gradient (parameters, inputs, initial state) to 1e-12."""
    torch.manual_seed(B + T)
    net = D.Net(S, A, D_hidden=H).double()
    ref = copy.deepcopy(net.lstm)
    g = torch.Generator().manual_seed(5)
    x, h, c = (torch.randn(*s, generator=g, dtype=torch.float64) for s in ((B, T, H + A), (B, H), (B, H)))
    G = torch.randn(B, T, H, generator=g, dtype=torch.float64)

    def run(fn, params):
        leaves = [v.clone().requires_grad_(True) for v in (x, h, c)]
        out, (h1, c1) = fn(*leaves)
        grads = torch.autograd.grad((out * G).sum() + h1.sum() + 2.0 * c1.sum(), leaves + list(params))
        return [out.detach(), h1.detach(), c1.detach()] + list(grads)

    ours = run(net.recur, net.lstm.parameters())
    theirs = run(lambda x_, h_, c_: (lambda o, hc: (o, (hc[0][0], hc[1][0])))(*ref(x_, (h_[None], c_[None]))), ref.parameters())
    assert len(ours) == len(theirs) == 10
    for a, b in zip(ours, theirs):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_truth_loss_is_the_learn_statement_from_the_q_tensors_on():
    """r2d2_truth.loss (numpy, time-major, what the kernel is held to) against r2d2_truth.learn (torch autograd, the reference's lines) in float64
    on one small batch: target, |td|, priority, loss, max_Q and d(loss)/dq."""
    seq, burn, n, B, H, S, A = 6, 3, 2, 7, 36, 5, 5
    torch.manual_seed(0)
    net, tgt = D.Net(S, A, D_hidden=H).double(), D.Net(S, A, D_hidden=H).double()
    rs = np.random.RandomState(0)
    b = D.batch(rs, B, seq, n, S, A, H, pad_rows=(B - 1,), done_rows=(0,))
    w = rs.uniform(0.2, 1.0, size=B).astype(np.float32)
    # gradient of the loss with respect to q_pred, through a hook on the truth's own output
    out = D.learn(net, tgt, b, w, seq, burn, n, D.GAMMA, 0.9, D.ALPHA)
    tm = lambda v: v.float().numpy().transpose(1, 0, 2)
    t = D.loss(tm(out["q_pred"]), tm(out["next_q"]), tm(out["next_target_q"]), b["action"], b["reward"], b["done"], w, burn, n, D.GAMMA, 0.9, D.ALPHA)
    scale = float(out["target_q"].abs().max())
    for key, mine in (("target_q", t["target_q"]), ("td_error", t["td"])):
        assert np.abs(mine - out[key][..., 0].numpy()).max() <= 1e-6 * scale, key  # (the q tensors went through float32 on the way)
    assert np.abs(t["priority"] - out["priority"][:, 0].numpy()).max() <= 1e-6 * scale ** D.ALPHA
    assert abs(t["loss"] - out["loss"]) <= 1e-6 * scale ** 2 and abs(t["max_Q"] - out["max_Q"]) <= 1e-6 * scale


def test_no_sweep_case_sits_on_a_discontinuity():
    """The loss kernel's sweep: no row with a near-tie of the two best next actions (the argmax would be decided by rounding), no |td| at its
    kink, an episode end inside row 0's trained window, the last row zero-padded into its trained window."""
    n_cases = 0
    for (B, T, A), (n_step, scale, eta) in ((s, v) for s in D.SWEEP_SHAPES for v in D.SWEEP_VARIANTS):
        c = D.sweep_case(B, T, A, n_step, scale)
        t = D.sweep_truth(c, eta)
        big = max(np.abs(t["target_q"]).max(), np.abs(t["q_taken"]).max())
        assert (t["gap"] > 2.0 ** -20 * np.abs(c["next_q"]).max()).all(), (B, T, A, n_step, scale)
        # |td| is continuous; its kink decides the SIGN of the last step's gradient: keep that step further from it than the tolerance reaches
        assert (t["td"][:, -1] > 2e-5 * big).all(), (B, T, A, n_step, scale)
        assert c["done"][0, c["burn"]:].any()
        if B > 1:
            assert c["pad"] > c["burn"] and not c["action"][B - 1, :c["pad"]].any() and not c["reward"][B - 1, :c["pad"]].any() and not c["done"][B - 1, :c["pad"]].any()
        n_cases += 1
    assert n_cases == 18 * 12
    sizes = {k: sorted({s[i] for s in D.SWEEP_SHAPES}) for i, k in enumerate("BTA")}
    assert sizes == {"B": [1, 7, 64], "T": [1, 3, 40], "A": [2, 5]}
    assert sorted({v[0] for v in D.SWEEP_VARIANTS}) == [1, 3] and sorted({v[1] for v in D.SWEEP_VARIANTS}) == [0.05, 50.0] and sorted({v[2] for v in D.SWEEP_VARIANTS}) == [0.0, 0.9, 1.0]


TOL = 1e-5  # the GPU tests' tolerance: the sensitivity conditions below are stated against it


def _off_every_discontinuity(c, t, what, tie_rows=()):
    """test_no_sweep_case_sits_on_a_discontinuity's conditions on one case; `tie_rows` hold an exact tie instead of a gap (an exact tie is not
    decided by rounding: the kernel documents the first maximum).  -> the scale the GPU criteria divide by."""
    B, tie = c["B"], list(tie_rows)
    big = max(np.abs(t["target_q"]).max(), np.abs(t["q_taken"]).max())
    free = np.ones(B, bool)
    free[tie] = False
    assert (t["gap"][free] > 2.0 ** -20 * np.abs(c["next_q"]).max()).all(), what
    assert (t["gap"][tie] == 0.0).all(), what
    assert (t["td"][:, -1] > 2e-5 * big).all(), what
    assert c["done"][0, c["burn"]:].any(), what
    if B > 1:
        assert c["pad"] > c["burn"] and not c["action"][B - 1, :c["pad"]].any() and not c["reward"][B - 1, :c["pad"]].any() and not c["done"][B - 1, :c["pad"]].any(), what
    return big


def test_no_edge_loss_case_sits_on_a_discontinuity():
    """EDGE_LOSS_CASES at both |Q| scales, and every targeted variant of EDGE_MULTI, under the conditions of the sweep; the table's coverage:
    every wave-count edge up to the cap of 1024 rows, A up to 64, T' + burn-in = 128, n_step > T' and n_step = 128."""
    cases = D.EDGE_LOSS_CASES
    for B, T, A, n_step, seed in cases:
        assert D.SWEEP_BURN + T <= 128 and B <= 1024 and A <= 64 and n_step <= 128
        for scale in D.EDGE_SCALES:
            c = D.sweep_case(B, T, A, n_step, scale, seed)
            _off_every_discontinuity(c, D.sweep_truth(c, D.EDGE_ETA), (B, T, A, n_step, scale))
    assert sorted({c[0] for c in cases}) == [2, 7, 64, 65, 128, 255, 256, 257, 1023, 1024]
    assert {c[0] for c in cases if c[1] <= 3} >= {65, 128, 255, 256, 257, 1023, 1024}
    assert sorted({c[2] for c in cases}) == [2, 5, 18, 64] and sorted({c[1] for c in cases}) == [1, 3, 40, 126] and sorted({c[3] for c in cases}) == [1, 3, 5, 128]
    shapes = {c[:3] for c in cases}
    assert {(1024, 1, 64), (255, 3, 64), (64, 40, 64), (256, 40, 5)} <= shapes
    assert {c[0] for c in cases if c[1] + D.SWEEP_BURN == 128} == {2, 65}
    assert {c[1] for c in cases if c[3] == 5} == {1, 3} and (7, 1, 2, 128) in {c[:4] for c in cases}
    assert D.EDGE_MULTI in cases and D.EDGE_MULTI[0] == 1024 and D.EDGE_SCALES == (0.05, 50.0) and D.EDGE_ETA == 0.9
    for scale in D.EDGE_SCALES:
        names = []
        for name, c, info in D.edge_multi_variants(scale):
            t = D.sweep_truth(c, D.EDGE_ETA)
            big = _off_every_discontinuity(c, t, (name, scale), info.get("tie_rows", ()))
            names.append(name)
            if "columns" in info:  # out-of-range actions over the whole trained window, both sides of the range
                window = c["action"][list(info["columns"]), c["burn"]:c["burn"] + c["T"]]
                assert ((window < 0) | (window >= c["A"])).all() and set(info["columns"].values()) == {0, c["A"] - 1}
            if "tie_rows" in info:  # the other maximum would move every tied row's |td| by far more than the tolerance
                other = D._copy(c)
                for row in info["tie_rows"]:
                    for s in range(c["T"]):
                        lo, hi = np.flatnonzero(c["next_q"][s, row] == c["next_q"][s, row].max())
                        other["next_target_q"][s, row, [lo, hi]] = c["next_target_q"][s, row, [hi, lo]]
                moved = np.abs(D.sweep_truth(other, D.EDGE_ETA)["td"] - t["td"]).max(1)
                assert (moved[list(info["tie_rows"])] > 100 * TOL * big).all() and set(info["tie_rows"]) & {64 * 15 + k for k in range(64)}
            if "done_row" in info:  # the target is the rescaled reward of the step itself
                r = c["reward"][info["done_row"], c["burn"]:c["burn"] + c["T"]].astype(np.float64)
                assert np.abs(t["target_q"][info["done_row"]] - D.val_rescale(r, float(np.float32(D.EPS)))).max() <= 1e-12
        assert len(names) == len(set(names)) == 8


def test_edge_loss_cases_would_expose_a_kernel_that_loses_waves():
    """Conditions on the inputs, from the float64 truth alone.  A sum over the first wave's rows only (what thread 0 holds before the cross-wave
    half of the block sum) misses every multi-wave case's loss by more than the loss criterion allows; in the one-weight variants it is zero;
    in the max_Q variants the maximum over every wave but the doctored row's own misses max_Q outright."""
    n = 0
    for B, T, A, n_step, seed in D.EDGE_LOSS_CASES:
        if B <= 64:
            continue
        for scale in D.EDGE_SCALES:
            c = D.sweep_case(B, T, A, n_step, scale, seed)
            t = D.sweep_truth(c, D.EDGE_ETA)
            big = max(np.abs(t["target_q"]).max(), np.abs(t["q_taken"]).max())
            first_wave = float((c["weights"].astype(np.float64) * t["td"][:, -1] ** 2)[:64].sum()) / B
            assert abs(first_wave - t["loss"]) > 10 * TOL * big * big, (B, T, A, n_step, scale)
            n += 1
    assert n == 2 * 10
    for scale in D.EDGE_SCALES:
        for name, c, info in D.edge_multi_variants(scale):
            t = D.sweep_truth(c, D.EDGE_ETA)
            big = max(np.abs(t["target_q"]).max(), np.abs(t["q_taken"]).max())
            if "only_row" in info:
                assert info["only_row"] >= 64 and t["loss"] > 10 * TOL * big * big, (name, scale)
                assert np.count_nonzero(t["grad_q"]) == 1
            if "max_q" in info:
                others = np.ones(c["B"], bool)
                others[info["row"] // 64 * 64:info["row"] // 64 * 64 + 64] = False
                assert t["max_Q"] == float(info["max_q"]) and t["q_taken"][others].max() < t["max_Q"], (name, scale)


def test_edge_step_shapes_would_expose_a_lost_k_chunk_or_unit_tile():
    """EDGE_STEP_SHAPES covers the rows and the H values of the kernel's dispatch edges, and its inputs are sensitive to them: where the last
    16-deep k chunk is partial, or the chunk count is no multiple of the four waves, a float64 cell without that chunk's share of h W_hh^T is
    further than TOL max|h'| from the truth, in every non-empty group; the same with the recurrent term of the last unit tile zeroed."""
    shapes = D.EDGE_STEP_SHAPES
    assert {s[0] for s in shapes} == {1, 15, 16, 17, 33} and sorted({s[1] for s in shapes}) == [8, 16, 20, 48, 52, 68, 100, 1024]
    for H in {s[1] for s in shapes}:
        assert {s[0] for s in shapes if s[1] == H} & {15, 16, 17}, H
    assert (17, 1024, 2) in shapes and any(s[0] == 33 and 48 <= s[1] <= 100 for s in shapes)
    assert sorted({-(-s[1] // 16) for s in shapes}) == [1, 2, 3, 4, 5, 7, 64]
    n = 0
    for rows, H, A in shapes:
        chunks = -(-H // 16)
        if H % 16 == 0 and chunks % 4 == 0:
            continue
        n += 1
        k0 = u0 = 16 * (chunks - 1)
        for s, g in enumerate(D.edge_step_groups(rows, H, A)):
            if not g["h"].shape[0]:
                continue
            exact = D.lstm_cell(g["xproj"], g["h"], g["c"], g["w_hh"])[0]
            h_cut = g["h"].clone()
            h_cut[:, k0:] = 0.0
            w_cut = g["w_hh"].clone()
            w_cut.view(4, H, H)[:, u0:, :] = 0.0
            for what, other in (("k chunk", D.lstm_cell(g["xproj"], h_cut, g["c"], g["w_hh"])[0]), ("unit tile", D.lstm_cell(g["xproj"], g["h"], g["c"], w_cut)[0])):
                assert float((other - exact).abs().max()) > 10 * TOL * float(exact.abs().max()), (rows, H, s, what)
    assert n == len(shapes) - 1  # all but H = 1024


def test_stable_inverse_rescale_is_the_written_one_in_float64_and_float32_as_written_is_not():
    """The departure of jh_r2d2_loss: y / (sqrt(1 + y) + 1) for sqrt(1 + y) - 1.  In float64 both forms agree to 1e-12; the reference's float32
    expression is off by more than 1e-5 of the value at |Q| = 0.05 -- which is why the kernel is held to float64 and not to float32 torch."""
    x = np.linspace(-0.05, 0.05, 41)[np.abs(np.linspace(-0.05, 0.05, 41)) > 1e-3]
    written = D.inv_val_rescale(x)
    y = 4 * 1e-3 * (np.abs(x) + 1 + 1e-3)
    u = y / (np.sqrt(1 + y) + 1) / (2 * 1e-3)
    stable = (x / (np.abs(x) + 1e-10)) * (u * u - 1)
    assert np.abs(stable - written).max() <= 1e-12
    as32 = D.inv_val_rescale(torch.as_tensor(x, dtype=torch.float32)).double().numpy()
    assert np.abs(as32 - written).max() / np.abs(written).max() > 1e-5


def test_param_count_is_the_padded_sum_of_the_segments():
    """jh_r2d2net_param_count_for is host-only: the sum over the 16 tensors of rows * cols rounded up to 4 floats."""
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    lib = _lib.load()
    up4 = lambda x: (x + 3) // 4 * 4
    lin = lambda out, inp: [(out, inp), (1, out)]
    for S, H, A in ((3, 8, 2), (5, 36, 5), (4, 512, 2)):
        shapes = lin(H, S) + [(4 * H, H + A), (4 * H, H), (1, 4 * H), (1, 4 * H)] + lin(H, H) + lin(H, H) + lin(H, H) + lin(A, H) + lin(1, H)
        assert lib.jh_r2d2net_param_count_for(S, H, A) == sum(up4(r * c) for r, c in shapes), (S, H, A)
    assert lib.jh_r2d2net_param_count_for(3, 6, 2) == -1 and lib.jh_r2d2net_param_count_for(3, 8, 1) == -1


def test_agent_raises_without_a_gpu_or_on_an_ineligible_configuration():
    from jorldy_amd.core.agent import Agent

    with pytest.raises(ValueError, match="R2D2 runs on libjorldy_hip only"):
        Agent("r2d2", state_size=(4, 84, 84), action_size=4, head="cnn")


# ---------------------------------------------------------------------------------------------- against the reference's recorded output
def test_fixtures_hold_what_the_generator_asserts():
    for name in D.FIXTURES:
        f = D.Fixture(name)
        assert (f.name == "r2d2_cartpole") == (f.q_scale == 1.0) and 0.0 < f.ref_target_err < (1e-3 if f.q_scale == 1.0 else 0.5e-5)
        for k in range(2):
            rec = f.learn(k)
            assert float(np.abs(rec["learn/target_q"]).max()) >= (5.0 if f.q_scale != 1.0 else 0.5)
            assert rec["learn/done"][:, f.n_burn_in:].any() and rec["learn/indices"].shape == (f.B,)
            top = np.sort(rec["learn/next_q"].astype(np.float64), -1)
            assert ((top[..., -1] - top[..., -2]) > 2.0 * 2.0 ** -24 * np.abs(rec["learn/next_q"]).max()).all()
        assert bool(f.z["rows/padded"].any()) == bool(f.zero_padding)


@pytest.mark.parametrize("name", ("r2d2", "r2d2_odd"))
def test_truth_reproduces_the_fixtures_tapped_quantities(name):
    """r2d2_truth.learn in float64, from the fixture's starting weights on the batch the reference sampled (the stored rows at the recorded
    indices), against what the reference's learn() held in front of its optimizer step: q, q_pred, both next-Q tensors, target_q, td_error,
    priority, p_j, the loss, and the gradients, each at 1e-5 of its largest entry.
    Not replayed: the second learn (it starts from the first one's stepped weights, which the fixture holds thinned; only the recipe's starting
    weights can be regenerated in full), and r2d2_cartpole's network half (its rows are thinned to fit the size cap: see the next test)."""
    f = D.Fixture(name)
    rows, rec = f.rows(), f.learn(0)
    assert rows is not None
    first_leaf = 256 - 1
    pick = rec["learn/indices"].astype(np.int64) - first_leaf
    b = {k: v[pick] for k, v in rows.items()}
    assert np.array_equal(b["reward"], rec["learn/reward"]) and np.array_equal(b["done"], rec["learn/done"])
    nets = []
    for which in (0, 1):
        m = D.Net(f.S, f.A, D_hidden=f.H).double()
        m.load_state_dict({k: v.double() for k, v in f.weights(which).items()})
        nets.append(m)
    t = D.learn(nets[0], nets[1], b, rec["learn/weights"], f.seq_len, f.n_burn_in, f.n_step, np.float32(f.gamma), np.float32(f.eta), np.float32(f.alpha))
    rel = lambda a, ref: float(np.abs(np.asarray(a, dtype=np.float64).reshape(ref.shape) - ref).max() / np.abs(ref).max())
    # (the reference's local `priority` is the value before the power, p_j after it: the truth returns the latter)
    for key, mine in (("q", t["q"]), ("q_pred", t["q_pred"]), ("next_q", t["next_q"]), ("next_target_q", t["next_target_q"]), ("target_q", t["target_q"]),
                      ("td_error", t["td_error"]), ("p_j", t["priority"])):
        assert rel(mine.numpy(), rec["learn/" + key].astype(np.float64)) <= 1e-5, key
    assert abs(t["loss"] - float(rec["learn/loss"])) <= 1e-5 * abs(float(rec["learn/loss"]))
    grads = {k: p.grad.numpy() for k, p in nets[0].named_parameters()}
    norm = np.sqrt(sum(float((g ** 2).sum()) for g in grads.values()))
    coef = min(1.0, f.clip_grad_norm / (norm + 1e-6))  # the fixture holds p.grad in front of optimizer.step(): after clip_grad_norm_
    assert abs(coef * norm - float(rec["grad_norm"])) <= 1e-5 * float(rec["grad_norm"])
    for k, g in grads.items():
        assert np.abs(f.thin(coef * g) - rec["grad_thin/" + k]).max() <= 1e-5 * float(rec["grad_absmax/" + k]) + 1e-12, k


def test_truth_loss_reproduces_the_cartpole_fixture_within_the_references_own_error():
    """r2d2_cartpole keeps its rows thinned (64 rows of four 512-wide states would be 0.5 MB), so the batch cannot be rebuilt and the network
    half of the truth is not replayed at H 512: the float64 loss statement starts from the recorded Q tensors.  target_q, td_error, p_j and the
    loss within 2 x hyper/ref_target_err + 1e-5 (8.9e-5 at the recorded 3.97e-5) of the largest target, both learns."""
    f = D.Fixture("r2d2_cartpole")
    for k in range(2):
        rec = f.learn(k)
        tm = lambda v: rec["learn/" + v].transpose(1, 0, 2)
        action = np.zeros(rec["learn/reward"].shape[:2], np.float32)  # learn() holds the first seq_len columns; the fold reads no action beyond them
        action[:, :f.seq_len] = rec["learn/action"][..., 0]
        t = D.loss(tm("q_pred"), tm("next_q"), tm("next_target_q"), action, rec["learn/reward"], rec["learn/done"], rec["learn/weights"], f.n_burn_in, f.n_step,
                   f.gamma, f.eta, f.alpha)
        big = float(np.abs(t["target_q"]).max())
        assert np.abs(t["target_q"] - rec["learn/target_q"][..., 0]).max() <= f.target_tol * big
        assert np.abs(t["td"] - rec["learn/td_error"][..., 0]).max() <= f.target_tol * big
        assert np.abs(t["priority"] - rec["learn/p_j"][:, 0]).max() <= f.target_tol * big ** f.alpha * 2
        assert abs(t["loss"] - float(rec["learn/loss"])) <= 2 * f.target_tol * big * float(np.abs(t["td"]).max())
