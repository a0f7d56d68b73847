"""R2D2's batched actors (csrc/jh_r2d2_actors.hip through ops.R2D2ActorFeed) at the kernel's own limits, against the host model of
tests/r2d2_actors_truth.py: N interact_callback state machines in float64 and decide().  Every case injects a trace and compares, per tick,
the row count, every copied column bit for bit and the priority within twice the case's own measured q rounding gap.  What each schedule
reaches is asserted without a GPU in tests/test_r2d2_actors_cpu.py."""
import numpy as np
import pytest
import torch

import margins
import r2d2_actors_truth as T
from tests.util import f32, npy

pytestmark = pytest.mark.gpu
SENTINEL = -7.5


def _ids(cases):
    return [c.name for c in cases]


def _feed(c):
    from jorldy_amd import ops

    return ops.R2D2ActorFeed(c.N, c.S, c.A, c.H, c.seq, c.burn, c.n, c.period, c.pad, c.gamma, c.eta, "cuda:0")


def _draws(tr, t):
    """The tick's (eps, u, rand_action): the trace's own, or eps = 1 > u = 0, which forces the injected action."""
    if "eps" in tr:
        return tr["eps"][t], tr["u"][t], tr["rand"][t]
    N = tr["done"].shape[1]
    return np.ones(N, np.float32), np.zeros(N), tr["action"][t]


class Run:
    """One feed driven through a case's trace; the rows held since the last restart are compared as whole columns."""

    def __init__(self, c, cap, feed=None, rows=None, obs_of=f32):
        self.c, (self.tr, self.truth) = c, T.built(c)
        self.feed = _feed(c) if feed is None else feed
        self.rows = self.feed.rows(cap) if rows is None else rows
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.act_out = (torch.zeros(c.N, dtype=torch.int64, device="cuda"), torch.zeros(c.N, dtype=torch.float32, device="cuda"))
        self.obs_of, self.held, self.kept, self.worst = obs_of, 0, [], 0.0

    def fresh_feed(self):
        """The state moves into a new object, which carries on."""
        saved = self.feed.state()
        self.feed = _feed(self.c)
        self.feed.load_state(saved)

    def act(self, t, h_in=None, c_in=None):
        tr, c = self.tr, self.c
        eps, u, ra = _draws(tr, t)
        self.feed.act(f32(tr["q"][t]), self.obs_of(tr["obs"][t]), f32(tr["h"][t]) if h_in is None else h_in, f32(tr["c"][t]) if c_in is None else c_in,
                      self.act_out, eps=eps, u=u, rand_action=ra)

    def emit(self, t, restart):
        self.feed.emit(self.tr["reward"][t], self.tr["done"][t], self.rows, self.count, restart=restart)
        torch.cuda.synchronize()

    def check_decision(self, t):
        q32 = self.tr["q"][t].astype(np.float32)
        action, q_taken = T.decide(q32, *_draws(self.tr, t))
        assert np.array_equal(action, self.tr["action"][t])
        assert np.array_equal(npy(self.act_out[0]), action) and np.array_equal(npy(self.act_out[1]), q_taken), f"tick {t}: action and q taken"

    def compare(self, lo, want, what):
        n = want["priority"].shape[0]
        for k in T.COLS[:-1]:
            got = npy(self.rows[k][lo:lo + n]).astype(np.float64)
            assert got.shape == want[k].shape and np.array_equal(got, want[k]), f"{what}: {k}"
        self.worst = max(self.worst, float(np.abs(npy(self.rows["priority"][lo:lo + n]) - want["priority"].reshape(-1)).max()))

    def check_held(self, what):
        """Every row since the last restart is still what it was when it was written."""
        if self.kept:
            self.compare(0, {k: np.concatenate([w[k] for w in self.kept]) for k in T.COLS}, what)

    def tick(self, t, restart, between=None, **act_kw):
        if restart:
            self.check_held(f"before the restart at tick {t}")
            self.held, self.kept = 0, []
        self.act(t, **act_kw)
        if between is not None:
            between()
        self.emit(t, restart)
        self.check_decision(t)
        want = T.rows_by_tick(self.truth[t])
        n = 0 if want is None else want["priority"].shape[0]
        assert int(self.count.item()) == self.held + n, f"tick {t}: rows emitted"
        if n:
            self.compare(self.held, want, f"tick {t}")
            self.kept.append(want)
        self.held += n

    def finish(self):
        self.check_held("at the end")
        c = self.c
        print(f"{c.name}: largest |priority - float64 host priority| = {self.worst:.3e} (allowed {T.tol(c):.3e} = 2 x the measured q rounding gap)")
        margins.leq(self.worst, T.tol(c), f"{c.name} actor-side priority vs the float64 host value")


def _run(c, restart_every=8, **kw):
    run = Run(c, restart_every * c.N, **kw)
    for t in range(c.ticks):
        run.tick(t, t % restart_every == 0)
    run.finish()
    return run


@pytest.mark.parametrize("c", T.COMPACTION, ids=_ids(T.COMPACTION))
def test_rows_are_compacted_in_actor_order_at_every_ballot_and_group_size(c):
    """N = 1, 16, 17, 64, 65, 130, 1024: one to sixteen ballots of the emit kernel's prefix with a partial last one, whole and partial
    16-actor groups of the act kernel.  Rows of a tick stand in ascending actor order behind the rows held; a restart every 8 ticks."""
    _run(c)


@pytest.mark.parametrize("c", T.GEOMETRY, ids=_ids(T.GEOMETRY))
def test_windows_at_the_largest_and_smallest_geometry(c):
    """seq_len + n_step = 160 (accepted, and the size of the emit kernel's LDS arrays) with 1, 88 and 155 trained steps, and L = 2;
    store_period 0, 1, between and past L; more than 2 L ticks, so the rings wrap and emit with a head that is not 0."""
    assert c.seq + c.n in (2, 160)
    _run(c)


def _offset_by_4_bytes(a):
    """A contiguous device copy of `a` that starts 4 bytes into its allocation."""
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(f32(a))
    return v


class _Spy:
    """The library, with the observation pointers jh_r2d2_actors_act receives recorded."""

    def __init__(self, lib):
        self._lib, self.obs = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "jh_r2d2_actors_act":
            return fn

        def act(h, q, obs, *rest):
            self.obs.append(obs.value)
            return fn(h, q, obs, *rest)

        return act


@pytest.mark.parametrize("c", T.WIDTH, ids=_ids(T.WIDTH))
def test_every_copy_width(c):
    """H / 4 = 1, 17 and 257 float4 per state row (one, one past the act kernel's 16 lanes, one past the emit kernel's 256); S = 1, 3
    (scalars), 4 and 152 (float4; L * S / 4 = 266 is past 256 lanes); A = 2, 5, 64; S = 8 from a tensor that is not 16-byte aligned
    (scalar reads into the ring, float4 from it)."""
    if c.name != "width-S8-unaligned":
        _run(c)
        return
    feed = _feed(c)
    feed.lib = spy = _Spy(feed.lib)
    _run(c, feed=feed, obs_of=_offset_by_4_bytes)
    assert len(spy.obs) == c.ticks and all(p % 16 == 4 for p in spy.obs), "jh_r2d2_actors_act read every observation from an unaligned tensor"


def test_unaligned_carried_state_is_refused_before_any_launch():
    """h_in / c_in are copied by float4 only: a tensor 4 bytes into its allocation is refused, and the object then runs its case from tick 0
    as if nothing had been asked of it."""
    from jorldy_amd._lib import JhError

    c = T.WIDTH[0]
    tr, _ = T.built(c)
    feed = _feed(c)
    out = (torch.zeros(c.N, dtype=torch.int64, device="cuda"), torch.zeros(c.N, dtype=torch.float32, device="cuda"))
    good, bad = f32(tr["h"][0]), _offset_by_4_bytes(tr["h"][0])
    assert bad.is_contiguous() and bad.data_ptr() % 16 == 4
    for h, cc in ((bad, good), (good, bad)):
        with pytest.raises(JhError):
            feed.act(f32(tr["q"][0]), f32(tr["obs"][0]), h, cc, out, eps=np.ones(c.N), u=np.zeros(c.N), rand_action=tr["action"][0])
    _run(c, feed=feed)


@pytest.mark.parametrize("c", T.DECISIONS, ids=_ids(T.DECISIONS))
def test_decisions_and_the_carried_state(c):
    """33 actors (two groups and one actor), A = 2 and 64, greedy / mixed / forced ticks: the action and q taken are decide()'s (first
    maximum, strict u < eps in double, clamped random action); the one-hot fed to the next tick is the action's, zero after a done; the
    carried h / c are what the step wrote, zero after a done; the emitted rows are the host's for decide()'s actions."""
    run = Run(c, 8 * c.N)
    tr, eye = run.tr, np.eye(c.A, dtype=np.float32)
    for t in range(c.ticks + 1):
        torch.cuda.synchronize()
        h_in, c_in, h_out, c_out, onehot = run.feed.carried()
        fresh = tr["done"][t - 1] if t else np.ones(c.N, bool)
        want = np.zeros((c.N, c.A), np.float32) if t == 0 else np.where(fresh[:, None], 0.0, eye[tr["action"][t - 1]])
        assert np.array_equal(npy(onehot), want), f"tick {t}: the one-hot fed"
        if t == c.ticks:
            assert np.array_equal(npy(h_in), np.where(fresh[:, None], 0.0, tr["hn"][t - 1])) and np.array_equal(npy(c_in), np.where(fresh[:, None], 0.0, tr["cn"][t - 1]))
            break
        assert np.array_equal(npy(h_in), tr["h"][t]) and np.array_equal(npy(c_in), tr["c"][t]), f"tick {t}: the carried state"
        assert not npy(h_in)[fresh].any() and not npy(c_in)[fresh].any()
        h_out.copy_(f32(tr["hn"][t]))  # what jh_r2d2net_act_step does between carried() and act()
        c_out.copy_(f32(tr["cn"][t]))
        run.tick(t, t % 8 == 0, h_in=h_in, c_in=c_in)
    run.finish()


@pytest.mark.parametrize("c", T.PRIORITY, ids=_ids(T.PRIORITY))
def test_priority_numerics(c):
    """|q| about 1e-3, 10 and 1e3 with exact zeros (the x / (|x| + 1e-10) factor at 0), rewards up to 100, a done at every fold position,
    (gamma, eta) = (0.997, 0.9), (1, 0), (0, 1), (0.99, 0.5)."""
    _run(c)


def test_rows_past_the_capacity_are_dropped_and_counted():
    """capacity = N = 5 and no restart between two emitting ticks: the count reports every row, the rows below the capacity are the host's
    in order, the N rows of memory behind the capacity keep their sentinel, and after a restart the actors carry on as the host's do (a
    dropped row's actor advanced like any other)."""
    c = T.CAPACITY[0]
    cap = c.N
    feed = _feed(c)
    big = feed.rows(cap + c.N)
    for v in big.values():
        v.fill_(SENTINEL)
    run = Run(c, cap, feed=feed, rows={k: v[:cap] for k, v in big.items()})
    t1, t2 = T.overflow_ticks(run.truth, cap)
    for t in range(t2):
        run.tick(t, restart=not t1 < t < t2)
    run.act(t2)
    run.emit(t2, restart=False)
    run.check_decision(t2)
    total = run.held + len(run.truth[t2])
    assert run.held < cap < total and int(run.count.item()) == total, "the count is over the capacity"
    want = T.rows_by_tick(run.truth[t2])
    run.compare(run.held, {k: v[:cap - run.held] for k, v in want.items()}, f"tick {t2}, the rows that fit")
    run.check_held("the first tick's rows")
    for k, v in big.items():
        assert bool((v[cap:] == SENTINEL).all()), f"{k}: memory behind the capacity"
    for t in range(t2 + 1, c.ticks):
        run.tick(t, restart=True)
    run.finish()
    for k, v in big.items():
        assert bool((v[cap:] == SENTINEL).all()), f"{k}: memory behind the capacity"


def test_save_and_load_on_an_even_and_an_odd_tick():
    """The state moves into a fresh object twice in one run: on an even tick that directly follows an emission, and on an odd one (the
    state blocks, the cursor and the carried state are double-buffered by tick parity).  Between act() and emit() it is refused."""
    from jorldy_amd._lib import JhError

    c = T.SAVELOAD[0]
    run = Run(c, 8 * c.N)
    even, odd = T.save_ticks(run.truth)
    assert even % 2 == 0 and odd % 2 == 1 and run.truth[even - 1]

    def refused():
        with pytest.raises(JhError, match="between"):
            run.feed.state()

    for t in range(c.ticks):
        if t in (even, odd):
            run.fresh_feed()
        run.tick(t, t % 8 == 0, between=refused if t == even + 1 else None)
    run.finish()
