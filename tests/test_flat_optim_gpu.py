"""The flat optimizer (csrc/jh_rbnet.hip: jh_rb_gradnorm_kernel + jh_rb_optim_kernel<Adam | RMSprop>; entered through jh_rbnet_optim_step by
ops.RainbowNet and through jh_flat_adam_step by ops.IQNNet / ops.R2D2Net) driven DIRECTLY: the starting state and the gradient are written
into the covered words of the flat buckets, one native [clip +] step runs, and all four buckets are read back.  No forward or backward pass
stands in front of it (section F excepted, whose subject is a tail of the backward pass inside the optimizer's launch).

Truth (tests/optim_truth.py): float64 torch.optim from the same state, fed OUR gradient as it sits in the bucket after the step -- with a clip
that is the clipped gradient -- must land where our weights and moments landed, by fp64_truth.check_flat_step's criteria
(2^-22 |w| + 1e-4 |dw| + 1e-6 lr per element; 1e-5 max |m| per moment).  The clip itself is checked apart from the step: the bucket against
coef64 * g, allowed max(1e-5, 2 x the error of torch-CPU float32's clip_grad_norm_) relative to max |g| (fp64_truth.vs_exact).

  A  size ladder: every rung of optim_truth.LADDER (test_flat_optim_cpu.py pins each to its launch edge), three forms
  B  step edges: late bias corrections; six un-forced steps (the device-side counter); set_lr in the middle; graph replay
  C  clip edges: inactive, biting, within 1e-3 of the norm, a norm near the 1e-6 guard, an all-zero gradient
  D  RMSprop without `centered` leaves m alone; centered RMSprop's first step
  E  padding words between segments stay zero (asserted in EVERY case here) -- also at test_netcore_gpu.py's shapes
  F  conv1's partial-sum tail inside the optimizer launch, with RMSprop
  G  the other owners of a hyper block and ticket: IQNNet, R2D2Net"""
import functools

import pytest
import torch

import fp64_truth as T
import optim_truth as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BUCKETS = ("params", "grads", "m", "v")
ADAM = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1.5e-4)        # config.rainbow.atari's eps, default betas
RMS_APEX = dict(lr=2.5e-4, beta1=0.95, beta2=0.999, eps=1.5e-7)  # Ape-X's RMSprop (beta1 = alpha)
HYPER = {"adam": ADAM, "rmsprop": RMS_APEX, "rmsprop_centered": RMS_APEX}


# ---------------------------------------------------------------------------------------------- nets, states, gradients
@functools.lru_cache(maxsize=None)
def _q(H, twin=0):
    """The ladder's net: RainbowNet kind "q", mlp head, S = 4, A = 2, max_batch 1 (n_params = H^2 + 8 H + 4).  Every test loads all four
    buckets and the hyper block before it steps, so an object is shared between tests; `twin` asks for a second one."""
    from jorldy_amd import ops

    return ops.RainbowNet(O.LADDER_S, O.LADDER_A, 1, H, "mlp", 1, DEV, kind="q")


def _mask(net):
    """True on the words a segment covers, False on the padding between segments."""
    mask = torch.zeros(net.n_params, dtype=torch.bool)
    for off, rows, cols in net.seg.values():
        mask[off : off + rows * cols] = True
    assert bool((~mask).any()), "this shape has no padding word"
    return mask


def _gradient(mask, seed, norm=None):
    """Magnitudes spread over four decades, both signs, a tenth exact zeros; zero on the padding.  norm: scaled to this 2-norm."""
    n, gen = mask.numel(), torch.Generator().manual_seed(seed)
    g = 10.0 ** (-4.0 * torch.rand(n, generator=gen, dtype=torch.float64)) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)
    g[torch.rand(n, generator=gen) < 0.1] = 0.0
    g[~mask] = 0.0
    if norm is not None:
        g = g * (norm / float(g.norm()))
    return g.float()


def _state(mask, seed, zero=False):
    """A non-zero optimizer state with v >= m^2 + 1e-3 (centered RMSprop takes sqrt(v - m^2): no cancellation to speak of), zero on the padding."""
    n, gen = mask.numel(), torch.Generator().manual_seed(1000 + seed)
    if zero:
        return dict(params=torch.zeros(n), m=torch.zeros(n), v=torch.zeros(n))
    w, m = 0.1 * torch.randn(n, generator=gen), 0.03 * torch.randn(n, generator=gen)
    v = m * m + 1e-3 + 1e-2 * torch.rand(n, generator=gen)
    return {k: torch.where(mask, t, torch.zeros(n)) for k, t in (("params", w), ("m", m), ("v", v))}


def _load(net, state, g, opt, hy, step):
    for k in ("params", "m", "v"):
        getattr(net, k).copy_(state[k])
    net.grads.copy_(g)
    net.set_hyper(hy["lr"], hy["beta1"], hy["beta2"], hy["eps"], step, centered=opt == "rmsprop_centered")


def _read(net):
    torch.cuda.synchronize()
    return {k: getattr(net, k).cpu().clone() for k in BUCKETS}


def _hyper_word(net, i):
    from jorldy_amd import ops

    torch.cuda.synchronize()
    return float(ops._wrap_device(net.hyper_ptr(), (16,), torch.float32, net.device, owner=net).cpu()[i])


def _native(opt):
    return "adam" if opt == "adam" else "rmsprop"


def _truth(opt, hy, state, step):
    return O.FlatTruth(opt, state["params"].numel(), hy["lr"], hy["beta1"], hy["beta2"], hy["eps"], params=state["params"], m=state["m"], v=state["v"], step=step)


def _padding_is_zero(after, mask, tag):
    for k in BUCKETS:
        assert not after[k][~mask].any(), f"{tag}: padding words of {k} were written"


def _check_clip(g, max_norm, g_after, tag):
    """The gradient bucket after a clipped step against coef64 * g, relative to max |g| (fp64_truth.vs_exact's rule)."""
    coef, _ = O.clip_coef64(g, max_norm)
    p32 = torch.nn.Parameter(torch.zeros_like(g))
    p32.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p32], max_norm)
    if coef == 1.0:
        assert torch.equal(g_after, g), f"{tag}: an inactive clip changed the gradient"
    return T.vs_exact(g_after, coef * g.double(), p32.grad, 1e-5, f"{tag} clipped gradient (coef {coef:.6f})")


def _forced_step(net, opt, step, clip=None, max_norm=None, seed=0, hy=None, zero_state=False, g=None, m_sentinel=None):
    """ONE native step from a given state at a given step count, checked against the float64 step of OUR gradient.  clip: max_norm as a
    multiple of the gradient's norm.  -> (the four buckets after the step, max_norm used)"""
    hy, mask = hy or HYPER[opt], _mask(net)
    state = _state(mask, seed, zero=zero_state)
    if m_sentinel is not None:
        state["m"] = torch.where(mask, torch.full_like(state["m"], m_sentinel), torch.zeros_like(state["m"]))
    g = _gradient(mask, seed) if g is None else g
    if clip is not None:
        max_norm = clip * float(g.double().norm())
    tag = f"{opt} n={net.n_params} step {step} clip {clip if max_norm is None or clip is not None else max_norm}"
    _load(net, state, g, opt, hy, step)
    net.optim_step(_native(opt), max_norm)
    after = _read(net)
    for k in BUCKETS:
        assert torch.isfinite(after[k]).all(), f"{tag}: {k} is not finite"
    if max_norm is None:
        assert torch.equal(after["grads"], g), f"{tag}: a step without a clip wrote the gradient bucket"
    else:
        _check_clip(g, max_norm, after["grads"], tag)
    truth = _truth(opt, hy, state, step)
    before, exact, _ = truth.step(after["grads"])
    truth.check(after, before, exact, tag)
    if opt == "rmsprop":
        assert torch.equal(after["m"], state["m"]), f"{tag}: RMSprop without `centered` wrote the m bucket"
    _padding_is_zero(after, mask, tag)
    if hasattr(net, "hyper_ptr"):
        assert _hyper_word(net, 4) == step + 1, f"{tag}: the step word"
    return after, max_norm


FORMS = [("adam", None), ("adam", 0.5), ("rmsprop_centered", 0.5)]
FORM_IDS = ["adam", "adam-clip", "rmsprop-centered-clip"]


# ---------------------------------------------------------------------------------------------- A: the size ladder
@pytest.mark.parametrize("opt,clip", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("H", list(O.LADDER))
def test_one_forced_step_at_every_rung_of_the_size_ladder(H, opt, clip):
    net = _q(H)
    assert net.n_params == H * H + 8 * H + 4
    _forced_step(net, opt, 3, clip=clip, seed=H)


# ---------------------------------------------------------------------------------------------- B: step edges
@pytest.mark.parametrize("step", [0, 1, 9, 999, 99999])
def test_adam_bias_corrections_late_in_training(step):
    _forced_step(_q(32), "adam", step, seed=step % 97, hy=dict(ADAM, lr=1e-3), zero_state=step == 0)


def _trajectory(net, opt, clip, steps=6, set_lr=None, seed=0):
    """`steps` consecutive native steps from a zero optimizer state (weights of ordinary size: their rounding is most of a step's error), a
    fresh gradient each, nothing re-imported: the kernel's own counter drives the bias corrections.  The float64 trajectory is fed the same
    bucket gradients; gradients are inputs, so a weight's error does not feed back and the allowance after step k is the running sum of the
    single-step allowances along the float64 trajectory (torch-CPU float32 stays at 0.19 to 0.24 of it over six steps).
    set_lr: (after step k, new rate)."""
    hy, mask = HYPER[opt], _mask(net)
    state = dict(_state(mask, 0, zero=True), params=_state(mask, seed)["params"])
    _load(net, state, torch.zeros(net.n_params), opt, hy, 0)
    truth = _truth(opt, hy, state, 0)
    allowed = torch.zeros(net.n_params, dtype=torch.float64)
    for k in range(1, steps + 1):
        g = _gradient(mask, seed + 10 * k)
        net.grads.copy_(g)
        max_norm = None if clip is None else clip * float(g.double().norm())
        net.optim_step(_native(opt), max_norm)
        after = _read(net)
        tag = f"{opt} clip {clip} un-forced step {k}"
        if max_norm is not None:
            _check_clip(g, max_norm, after["grads"], tag)
        before, exact, _ = truth.step(after["grads"])
        assert exact["step"] == k
        allowed += T.step_allowance(exact["params"], before["params"], truth.lr)
        truth.check(after, before, exact, tag, allowed=allowed.clone())
        _padding_is_zero(after, mask, tag)
        if hasattr(net, "hyper_ptr"):
            assert _hyper_word(net, 4) == k, f"{tag}: the step word"
        if set_lr is not None and k == set_lr[0]:
            net.set_lr(set_lr[1])
            truth.set_lr(set_lr[1])
            assert _hyper_word(net, 0) == torch.tensor(set_lr[1], dtype=torch.float32).item() and _hyper_word(net, 4) == k, "set_lr keeps the step count"


@pytest.mark.parametrize("opt,clip", FORMS, ids=FORM_IDS)
def test_six_unforced_steps_follow_the_float64_trajectory_and_count_themselves(opt, clip):
    _trajectory(_q(32), opt, clip)


def test_set_lr_in_the_middle_of_a_trajectory_applies_and_keeps_the_step_count():
    _trajectory(_q(32), "adam", 0.5, set_lr=(3, 1e-4), seed=3)


def test_clipped_step_under_graph_replay_is_byte_equal_to_eager_steps():
    """One clipped optim_step captured once and replayed four times, the gradient bucket refilled between replays, against four eager steps
    on a twin: every bucket byte for byte, and both step words 4 (the counter and its ticket live in device memory: a replay advances them)."""
    from jorldy_amd import ops

    a, b = _q(32), _q(32, twin=1)
    mask = _mask(a)
    state = _state(mask, 5)
    gs = [_gradient(mask, 50 + k) for k in range(4)]
    max_norm = 0.5 * min(float(g.double().norm()) for g in gs)  # bites at every replay
    _load(a, state, gs[0], "adam", ADAM, 0)
    a.optim_step("adam", max_norm)  # (warm-up outside the capture; the state is loaded again below)
    for net in (a, b):
        _load(net, state, gs[0], "adam", ADAM, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        a.optim_step("adam", max_norm)
    truth = _truth("adam", ADAM, state, 0)  # the eager twin's four steps are also followed in float64 (allowance: the running sum, as in _trajectory)
    allowed = torch.zeros(a.n_params, dtype=torch.float64)
    for g in gs:
        a.grads.copy_(g)
        graph.replay()
        b.grads.copy_(g)
        b.optim_step("adam", max_norm)
        ra, rb = _read(a), _read(b)
        for k in BUCKETS:
            assert torch.equal(ra[k], rb[k]), k
        before, exact, _ = truth.step(rb["grads"])
        allowed += T.step_allowance(exact["params"], before["params"], truth.lr)
        truth.check(ra, before, exact, "replayed step", allowed=allowed.clone())
    assert _hyper_word(a, 4) == 4 and _hyper_word(b, 4) == 4


# ---------------------------------------------------------------------------------------------- C: clip edges
CLIP_H = [32, 884]


@pytest.mark.parametrize("opt", ["adam", "rmsprop_centered"])
@pytest.mark.parametrize("H", CLIP_H)
def test_an_inactive_clip_is_byte_equal_to_no_clip(H, opt):
    """max_norm = 2 x the norm: the coefficient must be exactly 1 (and the norm launch in front must change nothing)."""
    a, b = _q(H), _q(H, twin=1)
    mask = _mask(a)
    state, g = _state(mask, 7), _gradient(mask, 7)
    _load(a, state, g, opt, HYPER[opt], 3)
    _load(b, state, g, opt, HYPER[opt], 3)
    a.optim_step(_native(opt), 2.0 * float(g.double().norm()))
    b.optim_step(_native(opt), None)
    ra, rb = _read(a), _read(b)
    for k in BUCKETS:
        assert torch.equal(ra[k], rb[k]), k
    assert torch.equal(ra["grads"], g) and not torch.equal(ra["params"], state["params"])
    assert _hyper_word(a, 4) == 4 and _hyper_word(b, 4) == 4


@pytest.mark.parametrize("clip", [0.5, 1.0 - 1e-3, 1.0 + 1e-3])
@pytest.mark.parametrize("H", CLIP_H)
def test_a_clip_that_bites_and_clips_within_a_thousandth_of_the_norm(H, clip):
    _forced_step(_q(H), "adam", 3, clip=clip, seed=11)


@pytest.mark.parametrize("H", CLIP_H)
def test_clip_of_a_norm_near_the_guard(H):
    """|g| = 1e-4 under max_norm 1e-5: coef = 1e-5 / (1e-4 + 1e-6), the guard is a 1 % effect."""
    net = _q(H)
    g = _gradient(_mask(net), 13, norm=1e-4)
    after, _ = _forced_step(net, "adam", 3, max_norm=1e-5, seed=13, g=g)
    got = float(after["grads"].double().norm()) / float(g.double().norm())
    assert abs(got * 1.01e-4 / 1e-5 - 1.0) < 1e-4, got  # 0.0990: with the guard; 0.1 without it


@pytest.mark.parametrize("opt", ["adam", "rmsprop_centered"])
@pytest.mark.parametrize("H", CLIP_H)
def test_an_all_zero_gradient_under_a_clip(H, opt):
    """coef = min(1, max_norm / 1e-6): nothing becomes non-finite (asserted in _forced_step); from a zero state the weights keep their bytes."""
    net = _q(H)
    zero = torch.zeros(net.n_params)
    for max_norm in (0.5, 1e-7):
        _forced_step(net, opt, 3, max_norm=max_norm, seed=17, g=zero)
    mask = _mask(net)
    state = _state(mask, 0, zero=True)
    state["params"] = _state(mask, 17)["params"]
    _load(net, state, zero, opt, HYPER[opt], 3)
    net.optim_step(_native(opt), 0.5)
    after = _read(net)
    assert torch.equal(after["params"], state["params"]) and not after["m"].any() and not after["v"].any() and not after["grads"].any()


# ---------------------------------------------------------------------------------------------- D: RMSprop forms
@pytest.mark.parametrize("alpha", [0.95, 0.99])
@pytest.mark.parametrize("H", [32, 724])
def test_rmsprop_without_centered_leaves_the_m_bucket_alone(H, alpha):
    """m holds a sentinel in every covered word; _forced_step asserts it byte-unchanged after the step."""
    for clip in (None, 0.5):
        after, _ = _forced_step(_q(H), "rmsprop", 3, clip=clip, seed=19, hy=dict(RMS_APEX, beta1=alpha), m_sentinel=-7.25)
        assert float(after["m"].min()) == -7.25


@pytest.mark.parametrize("alpha", [0.95, 0.99])
def test_centered_rmsprop_first_step_from_a_zero_state(alpha):
    """v - m^2 = a (1 - a) g^2 here: every weight with a gradient moves by lr / (sqrt(a (1 - a)) + eps / |g|), 4.6 lr at alpha 0.95."""
    _forced_step(_q(32), "rmsprop_centered", 0, seed=23, hy=dict(RMS_APEX, beta1=alpha), zero_state=True)


# ---------------------------------------------------------------------------------------------- E: padding at test_netcore_gpu.py's shapes
def _netcore(name):
    from jorldy_amd import ops

    if name == "iqn":
        return ops.IQNNet(3, 3, 5, 2, 8, 2, DEV)
    if name == "r2d2":
        return ops.R2D2Net(3, 3, 8, 2, 4, 1, 1, DEV)
    return ops.RainbowNet(3, 2, 3 if name == "rainbow" else 1, 8, "mlp", 2, DEV, kind=name)


@pytest.mark.parametrize("name", ["q", "dueling", "rainbow", "iqn", "r2d2"])
def test_padding_words_stay_zero_at_the_smallest_tables(name):
    """3 inputs, 8 wide: tables with padding (_mask asserts there is some, _forced_step that it is zero in all four buckets afterwards)."""
    net = _netcore(name)
    for opt, clip in FORMS if name in ("q", "dueling", "rainbow") else FORMS[:2]:
        _forced_step(net, opt, 3, clip=clip, seed=29)


# ---------------------------------------------------------------------------------------------- F: conv1's tail inside the optimizer launch
@pytest.mark.parametrize("centered", [False, True], ids=["plain", "centered"])
@pytest.mark.parametrize("frame", [(1, 36, 36), (4, 44, 52), (8, 36, 36)], ids=["cin1", "cin4", "cin8"])
def test_conv1_tail_in_the_optimizer_launch_with_rmsprop(frame, centered):
    """Twin CNN nets take two consecutive un-clipped RMSprop steps, one after backward(g, defer=True) -- conv1's weight gradient is still
    partial sums, which 64 Cin + 1 extra workgroups at the end of the optimizer's grid add up AND step -- the other after backward(g): every
    bucket byte-equal after each step, the step word 2 (grids of 512 + 257 and 512 + 513 workgroups: no multiple of 8, what the ticket's
    residue arithmetic is for).  The deferred twin's step is also checked as arithmetic against float64 from its own previous state.
    Cin = 1 takes conv1's weight gradient on the tile engine (the dedicated kernel wants Cin % 4 == 0), so nothing is deferred there: that
    case holds the two entries equal on the plain grid."""
    from jorldy_amd import ops

    A, K, H, B = 2, 3, 8, 2
    opt, hy = ("rmsprop_centered" if centered else "rmsprop"), RMS_APEX
    nets = [ops.RainbowNet(frame, A, K, H, "cnn", B, DEV, kind="rainbow") for _ in range(2)]
    mask = _mask(nets[0])
    gen = torch.Generator().manual_seed(31)
    state = _state(mask, 0, zero=True)
    state["params"] = torch.where(mask, 0.05 * torch.randn(mask.numel(), generator=gen), torch.zeros(mask.numel()))
    x = torch.randint(0, 256, (2 * B,) + frame, dtype=torch.uint8, generator=gen).cuda()
    noise = torch.randn(3, nets[0].noise_len, generator=gen).cuda()
    n_c1 = 32 * frame[0] * 64 + 32
    for net in nets:
        _load(net, state, torch.zeros(mask.numel()), opt, hy, 0)
    prev = state
    for k in (1, 2):
        gl = (0.05 * torch.randn(B, A, K, generator=gen)).cuda()
        out = torch.empty(3, B, A, K, device=DEV)
        for net, defer in zip(nets, (True, False)):
            net.learn_forward(x, B, noise, out)
            net.backward(gl, defer=defer)
            net.optim_step("rmsprop", None)
        ra, rb = _read(nets[0]), _read(nets[1])
        for name in BUCKETS:
            assert torch.equal(ra[name], rb[name]), (k, name)
        assert float(ra["grads"][:n_c1].abs().max()) > 0, "conv1's gradient is empty: the tail had nothing to do"
        assert _hyper_word(nets[0], 4) == k and _hyper_word(nets[1], 4) == k
        truth = _truth(opt, hy, prev, k - 1)
        before, exact, _ = truth.step(ra["grads"])
        truth.check(ra, before, exact, f"deferred conv1 tail, Cin {frame[0]}, {opt} step {k}")
        if not centered:
            assert not ra["m"].any()
        _padding_is_zero(ra, mask, f"conv1 tail step {k}")
        prev = ra


# ---------------------------------------------------------------------------------------------- G: the other owners
@pytest.mark.parametrize("name", ["iqn", "r2d2"])
def test_other_owners_forced_clipped_adam_step(name):
    _forced_step(_netcore(name), "adam", 3, clip=0.5, seed=37)


@pytest.mark.parametrize("name", ["iqn", "r2d2"])
def test_other_owners_count_their_own_steps_over_six_unforced_steps(name):
    """No hyper_ptr here: a counter that stalls or runs ahead shows as bias corrections of the wrong step (step 1 vs 2: the update is off by
    a factor 1.9 / 1.0 in m and 1.4 in sqrt(v))."""
    _trajectory(_netcore(name), "adam", 0.5, seed=41)
