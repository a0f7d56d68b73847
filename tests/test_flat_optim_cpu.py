"""The flat optimizer's float64 truth (tests/optim_truth.py) pinned against closed forms, the shared step criterion pinned against torch-CPU
float32 (an implementation it must let through) and against small arithmetic faults (which it must not), and the size ladder of
test_flat_optim_gpu.py pinned to the launch edges it is meant for.  No GPU: the library's host-only jh_rbnet_param_count_for gives the sizes."""
import math

import pytest
import torch

import optim_truth as O


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def _g(n, seed):
    gen = torch.Generator().manual_seed(seed)
    g = 10.0 ** (-4.0 * torch.rand(n, generator=gen)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    g[torch.rand(n, generator=gen) < 0.1] = 0.0
    return g.float()


# ---------------------------------------------------------------------------------------------- the truth vs closed forms
def test_first_adam_step_from_a_zero_state_moves_every_weight_by_lr_g_over_abs_g_plus_eps():
    n, lr, eps = 257, 1e-3, 1.5e-4
    g = _g(n, 1)
    w0 = torch.randn(n, generator=torch.Generator().manual_seed(2)).float()
    t = O.FlatTruth("adam", n, lr, eps=eps, params=w0)
    before, after, seen = t.step(g)
    assert torch.equal(seen, g.double()) and before["step"] == 0 and after["step"] == 1
    g64 = g.double()
    # m / bc1 = g, sqrt(v / bc2) = |g| exactly in real arithmetic; float64 leaves a few ulps
    torch.testing.assert_close(after["params"] - w0.double(), -lr * g64 / (g64.abs() + eps), rtol=1e-12, atol=0.0)
    assert not (after["params"] - w0.double())[g == 0].any()


@pytest.mark.parametrize("K", [1, 6, 40])
def test_constant_gradient_over_k_steps_gives_the_geometric_moments(K):
    n, b1, b2 = 64, 0.9, 0.999
    g = _g(n, 3)
    t = O.FlatTruth("adam", n, 1e-3, b1, b2)
    for _ in range(K):
        _, after, _ = t.step(g)
    g64 = g.double()
    assert after["step"] == K
    torch.testing.assert_close(after["m"], g64 * (1 - b1 ** K), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(after["v"], g64 * g64 * (1 - b2 ** K), rtol=1e-12, atol=0.0)
    # and the float32 twin follows within float32
    torch.testing.assert_close(t.r32.state()["m"].double(), after["m"], rtol=1e-5, atol=0.0)


def test_first_centered_rmsprop_step():
    n, lr, a, eps = 129, 2.5e-4, 0.95, 1.5e-7
    g = _g(n, 4)
    t = O.FlatTruth("rmsprop_centered", n, lr, a, eps=eps)
    _, after, _ = t.step(g)
    g64 = g.double()
    torch.testing.assert_close(after["m"], (1 - a) * g64, rtol=1e-12, atol=0.0)
    torch.testing.assert_close(after["v"], (1 - a) * g64 * g64, rtol=1e-12, atol=0.0)
    # sqrt(v - m^2) = |g| sqrt((1 - a) - (1 - a)^2) = |g| sqrt(a (1 - a))  (0.218 |g| at Ape-X's alpha)
    torch.testing.assert_close(after["params"], -lr * g64 / (g64.abs() * math.sqrt(a * (1 - a)) + eps), rtol=1e-10, atol=0.0)
    plain = O.FlatTruth("rmsprop", n, lr, a, eps=eps)
    _, after_p, _ = plain.step(g)
    assert after_p["m"] is None
    torch.testing.assert_close(after_p["params"], -lr * g64 / (g64.abs() * math.sqrt(1 - a) + eps), rtol=1e-10, atol=0.0)


def test_clip_coefficient_of_a_hand_made_gradient():
    g = torch.zeros(8)
    g[1], g[6] = 3.0, -4.0  # norm 5
    coef, norm = O.clip_coef64(g, 2.0)
    assert norm == 5.0 and coef == 2.0 / (5.0 + 1e-6)
    assert O.clip_coef64(g, 10.0)[0] == 1.0          # inactive: exactly 1
    assert O.clip_coef64(g, 5.0)[0] < 1.0            # max_norm = norm: the guard makes it bite
    assert O.clip_coef64(torch.zeros(8), 1e-7)[0] == 0.1  # an all-zero gradient under a max_norm below the guard
    assert O.clip_coef64(torch.zeros(8), 0.5)[0] == 1.0
    t = O.FlatTruth("adam", 8, 1e-3)
    _, _, seen = t.step(g, max_norm=2.0)
    torch.testing.assert_close(seen, g.double() * coef, rtol=1e-15, atol=0.0)
    _, _, seen = t.step(g, max_norm=10.0)
    assert torch.equal(seen, g.double())
    # near the guard: norm 1e-4, max_norm 1e-5 -> the + 1e-6 is a 1 % effect
    coef, norm = O.clip_coef64(g.double() * 2e-5, 1e-5)
    assert abs(norm - 1e-4) < 1e-18 and abs(coef - 1e-5 / 1.01e-4) < 1e-9 and abs(coef / (1e-5 / norm) - 1 / 1.01) < 1e-6


def test_a_given_state_and_step_count_are_where_the_step_starts():
    n, lr, b1, b2, eps, step = 33, 1e-3, 0.9, 0.999, 1e-8, 999
    gen = torch.Generator().manual_seed(5)
    w0, m0 = torch.randn(n, generator=gen), 0.01 * torch.randn(n, generator=gen)
    v0 = m0 * m0 + 1e-3 * torch.rand(n, generator=gen)
    g = _g(n, 6)
    t = O.FlatTruth("adam", n, lr, b1, b2, eps, params=w0, m=m0, v=v0, step=step)
    before, after, _ = t.step(g)
    assert before["step"] == step and after["step"] == step + 1 and torch.equal(before["params"], w0.double())
    m1 = b1 * m0.double() + (1 - b1) * g.double()
    v1 = b2 * v0.double() + (1 - b2) * g.double() ** 2
    want = w0.double() - lr / (1 - b1 ** (step + 1)) * m1 / ((v1 / (1 - b2 ** (step + 1))).sqrt() + eps)
    torch.testing.assert_close(after["params"], want, rtol=1e-12, atol=1e-18)
    torch.testing.assert_close(after["m"], m1, rtol=1e-12, atol=0.0)


# ---------------------------------------------------------------------------------------------- the criterion lets fp32 through and nothing else
def _state(n, seed):
    gen = torch.Generator().manual_seed(seed)
    w0, m0 = 0.1 * torch.randn(n, generator=gen), 0.03 * torch.randn(n, generator=gen)
    return w0, m0, m0 * m0 + 1e-3 + 1e-2 * torch.rand(n, generator=gen)


@pytest.mark.parametrize("opt,hy", [("adam", dict(lr=3e-4, eps=1.5e-4)), ("rmsprop_centered", dict(lr=2.5e-4, beta1=0.95, eps=1.5e-7)), ("rmsprop", dict(lr=2.5e-4, beta1=0.99, eps=1e-8))])
def test_torch_cpu_float32_passes_the_step_criterion_and_small_faults_do_not(opt, hy):
    n = 5000
    w0, m0, v0 = _state(n, 7)
    g = _g(n, 8)
    t = O.FlatTruth(opt, n, params=w0, m=m0, v=v0, step=3, **hy)
    before, after, _ = t.step(g)
    s32 = t.r32.state()
    ours = dict(params=s32["params"], m=s32["m"], v=s32["v"])
    assert t.check(ours, before, after, f"torch float32 {opt}") < 1.0
    # a step whose update is 0.1 % short (a bias correction or eps off by that much) does not pass
    short = dict(ours, params=before["params"] + 0.999 * (after["params"] - before["params"]))
    with pytest.raises(AssertionError):
        t.check(short, before, after, "short step")
    # nor does a second moment built with (1.f - beta) from the float32 beta (1.3e-5 relative at beta2 = 0.999)
    if opt == "adam":
        with pytest.raises(AssertionError):
            t.check(dict(ours, v=after["v"] * (1 + 1.3e-5)), before, after, "float beta")


# ---------------------------------------------------------------------------------------------- the size ladder
def test_every_rung_of_the_size_ladder_lies_on_its_side_of_its_edge(lib):
    e = O.edges()
    assert e["opt_pass"] == O.opt_wgs() * O.LANES == 131072 and e["norm_first_unroll"] == 196608 and e["norm_all_unroll"] == 262144, \
        "the launch constants moved (or JH_RB_OPTIM_GRID is set): re-derive the ladder"
    for H, (what, on_its_side) in O.LADDER.items():
        n = int(lib.jh_rbnet_param_count_for(2, 0, O.LADDER_S, 0, 0, H, O.LADDER_A, 1))
        assert n == H * H + 8 * H + 4, (H, n)
        assert n % O.VEC == 0, "the buckets are whole float4s: the scalar tails of both kernels never run"
        assert on_its_side(n // O.VEC, e), f"H = {H}: {n // O.VEC} float4s no longer reach '{what}'"


def test_the_optimizer_grid_is_read_like_the_library_reads_it():
    assert O.opt_wgs({}) == 512
    for env, want in (("1024", 1024), (" 64x", 64), ("abc", 0), ("", 0)):
        assert O.opt_wgs({"JH_RB_OPTIM_GRID": env}) == want, env
