"""Host model of R2D2's batched recurrent actors (csrc/jh_r2d2_actors.hip) and the case tables of its tests.

The truth is N independent R2D2.interact_callback state machines (jorldy_amd/core/agent/r2d2.py, numpy, float64 q and reward) fed an injected
trace, plus `decide`, a numpy restatement of the act kernel's decision rule.  Nothing here needs a GPU: tests/test_r2d2_actors_cpu.py measures
every recorded tolerance and asserts what each schedule reaches, tests/test_r2d2_actors_gpu.py and tests/test_r2d2_actors_edges_gpu.py drive
ops.R2D2ActorFeed with the same traces."""
import functools
from collections import deque, namedtuple

import numpy as np

COLS = ("state", "prev_action_onehot", "action", "reward", "done", "hidden_h", "hidden_c", "next_hidden_h", "next_hidden_c", "priority")


def host_actor(seq, burn, n, period, pad, gamma, eta):
    """An R2D2 that holds only what interact_callback reads: no device, no network."""
    from jorldy_amd.core.agent.r2d2 import R2D2

    ag = object.__new__(R2D2)
    ag.seq_len, ag.n_burn_in, ag.n_step, ag.store_period, ag.zero_padding, ag.gamma, ag.eta = seq, burn, n, period, pad, gamma, eta
    ag.tmp_buffer, ag.store_period_stamp, ag.store_start, ag.hidden, ag.prev_action = deque(maxlen=n + seq), 0, True, None, None
    return ag


def done_from_sets(sets, ticks):
    """[ticks, N] bool from one set of episode-end ticks per actor."""
    return np.asarray([[t in s for s in sets] for t in range(ticks)])


def done_schedule(seed, ticks, N, lo, hi, quiet=0):
    """[ticks, N] bool for many actors: every actor draws its own episode lengths from lo..hi (the first one `quiet` ticks longer), so the
    actors fall out of phase with each other within a few episodes."""
    rs = np.random.RandomState(seed)
    lengths = rs.randint(lo, hi + 1, size=(N, ticks))
    lengths[:, 0] += quiet
    ends = np.cumsum(lengths, axis=1) - 1
    done = np.zeros((ticks, N), bool)
    for a in range(N):
        done[ends[a][ends[a] < ticks], a] = True
    return done


def window_schedule(L, n, ticks):
    """[ticks, 3] bool for the long windows.  Actor 0 ends its first episode after 1.5 L ticks (the ring has wrapped by then), the next one
    n + 1 ticks later (the cut of the first lands on the end of the second) and one more at 2 L + 10; actor 1 ends episodes at ticks 3 and
    3 + n and at L / 2, then runs 1.5 L + 20 ticks without an end; actor 2 never ends one."""
    done = np.zeros((ticks, 3), bool)
    done[[L + L // 2, L + L // 2 + n + 1, 2 * L + 10], 0] = True
    done[[3, 3 + n, L // 2], 1] = True
    return done


def decide(q32, eps, u, rand_action):
    """The act kernel's rule for one tick.  q32 [N, A] float32; eps / u / rand_action [N] or all None (greedy) -> (action int64 [N],
    q_taken float32 [N]): the first maximum of the float32 q; the random action, clamped to 0..A-1, where u < float64(float32(eps))."""
    q32 = np.asarray(q32)
    assert q32.dtype == np.float32 and q32.ndim == 2
    N, A = q32.shape
    action = np.empty(N, np.int64)
    for a in range(N):
        best, act = q32[a, 0], 0
        for k in range(1, A):
            if q32[a, k] > best:
                best, act = q32[a, k], k
        action[a] = act
    if eps is not None:
        e = np.asarray(eps, dtype=np.float32).astype(np.float64)
        rnd = np.asarray(u, dtype=np.float64) < e
        action = np.where(rnd, np.clip(np.asarray(rand_action, dtype=np.int64), 0, A - 1), action)
    return action, q32[np.arange(N), action]


def trace(seed, ticks, N, S, A, H, done, q_scale=3.0, rewards=(-1.0, 0.0, 0.5, 1.0), zero_q=0.0):
    """The injected ticks: observations, all-action q in float64, the forced action, LSTM states, rewards, the done schedule [ticks, N].
    zero_q: the share of (tick, actor) q rows that are exactly zero."""
    rs = np.random.RandomState(seed)
    tr = dict(obs=rs.randn(ticks, N, S).astype(np.float32), q=q_scale * rs.randn(ticks, N, A), action=rs.randint(0, A, size=(ticks, N)),
              h=rs.randn(ticks, N, H).astype(np.float32), c=rs.randn(ticks, N, H).astype(np.float32),
              reward=rs.choice(list(rewards), size=(ticks, N)).astype(np.float32))
    if zero_q:
        tr["q"][rs.random_sample((ticks, N)) < zero_q] = 0.0
    tr["done"] = np.asarray(done, dtype=bool)
    assert tr["done"].shape == (ticks, N)
    return tr


def decision_trace(seed, ticks, N, S, A, H, done):
    """A trace whose actions are decide()'s.  Tick t is greedy (t % 3 == 0: eps = u = rand_action = None), mixed (t % 3 == 1) or forced
    (t % 3 == 2: eps = 1 > u = 0).  On a mixed tick actor a has, by a % 5: u far below eps; u == float64(float32(eps)); u the float64 just
    below it; u = the decimal eps was rounded from (below float32(0.3), above float32(0.7)); u far above eps.  Its q rows hold an exact tie
    of two maxima (a % 3 == 0), the maximum at A - 1 (a % 3 == 1) or a tie that includes A - 1 (a % 3 == 2); rand_action is -1 (a % 4 == 0),
    A (a % 4 == 1) or in range.  h / c are the carried state: hn / cn (what the LSTM step of tick t wrote) of the tick before, zero at the
    start and after a done."""
    tr = trace(seed, ticks, N, S, A, H, done)
    rs = np.random.RandomState(seed + 1)
    tr["hn"], tr["cn"] = rs.randn(ticks, N, H).astype(np.float32), rs.randn(ticks, N, H).astype(np.float32)
    tr["eps"], tr["u"], tr["rand"] = [None] * ticks, [None] * ticks, [None] * ticks
    for t in range(ticks):
        if t % 3 == 1:
            top = np.abs(tr["q"][t]).max(-1) + 1.0
            for a in range(N):
                j = rs.randint(0, A - 1)
                k = rs.randint(j + 1, A)
                if a % 3 == 0:
                    tr["q"][t, a, j] = tr["q"][t, a, k] = top[a]
                elif a % 3 == 1:
                    tr["q"][t, a, A - 1] = top[a]
                else:
                    tr["q"][t, a, j] = tr["q"][t, a, A - 1] = top[a]
            dec = np.where(np.arange(N) % 2 == 0, 0.3, 0.7)
            eps = dec.astype(np.float32)
            e = eps.astype(np.float64)
            u = np.select([np.arange(N) % 5 == i for i in range(5)], [0.01 * e, e, np.nextafter(e, 0.0), dec, 0.5 + 0.5 * e])
            ra = rs.randint(0, A, size=N)
            ra[np.arange(N) % 4 == 0], ra[np.arange(N) % 4 == 1] = -1, A
            tr["eps"][t], tr["u"][t], tr["rand"][t] = eps, u, ra
        elif t % 3 == 2:
            tr["eps"][t], tr["u"][t], tr["rand"][t] = np.ones(N, np.float32), np.zeros(N), tr["action"][t].copy()
        tr["action"][t], _ = decide(tr["q"][t].astype(np.float32), tr["eps"][t], tr["u"][t], tr["rand"][t])
        prev_done = tr["done"][t - 1][:, None] if t else np.ones((N, 1), bool)
        tr["h"][t] = np.where(prev_done, 0.0, tr["hn"][t - 1])
        tr["c"][t] = np.where(prev_done, 0.0, tr["cn"][t - 1])
    return tr


def host_rows(case, tr, gamma, eta, q_as=np.float64, ages=None):
    """rows[t] = [(actor, row dict)] in ascending actor order, from N interact_callbacks with float64 q / reward.
    case = (seq_len, n_burn_in, n_step, store_period, zero_padding, S, A); q_as: round the taken q to this type first.
    ages: a list that receives (tick, actor, records appended since the actor's window was last cut) per emitted row: above L, the deque
    has dropped entries, so a ring of L slots has wrapped."""
    seq, burn, n, period, pad, S, A = case
    ticks, N = tr["done"].shape
    actors, prev, rows = [host_actor(seq, burn, n, period, pad, gamma, eta) for _ in range(N)], [None] * N, []
    eye, age = np.eye(A, dtype=np.float32), [0] * N
    for t in range(ticks):
        out = []
        for a, ag in enumerate(actors):
            age[a], window = age[a] + 1, ag.tmp_buffer
            act = int(tr["action"][t, a])
            onehot = np.zeros((1, A), np.float32) if prev[a] is None else eye[[prev[a]]]
            row = ag.interact_callback({"state": tr["obs"][t, a][None], "reward": np.asarray([[tr["reward"][t, a]]], np.float64), "done": np.asarray([[tr["done"][t, a]]]),
                                        "action": np.asarray([[act]]), "prev_action_onehot": onehot, "q": np.asarray([[tr["q"][t, a, act]]]).astype(q_as).astype(np.float64),
                                        "hidden_h": tr["h"][t, a][None, None], "hidden_c": tr["c"][t, a][None, None]})
            prev[a] = None if tr["done"][t, a] else act
            if row:
                out.append((a, row))
                if ages is not None:
                    ages.append((t, a, age[a]))
            if ag.tmp_buffer is not window:  # cut after an episode end: the last n_step records stay
                age[a] = n
        rows.append(out)
    return rows


def rows_by_tick(rows_t):
    """One tick's [(actor, row dict)] -> {column: float64 array [rows, ...]} in ascending actor order (None when the tick emits nothing)."""
    if not rows_t:
        return None
    return {k: np.concatenate([np.asarray(r[k], dtype=np.float64) for _, r in rows_t], axis=0) for k in COLS}


def window_lengths(truth):
    """Per emitted row, the ticks its window holds: L for a full one, fewer when it is zero-padded at the front (observations are randn,
    never a zero row)."""
    return [int((r["state"][0] != 0).any(-1).sum()) for out in truth for _, r in out]


def overflow_ticks(truth, cap):
    """(t1, t2): the first two emitting ticks in a row of which the first leaves room (0 < rows < cap) and the second runs past `cap`."""
    emitting = [t for t, out in enumerate(truth) if out]
    for t1, t2 in zip(emitting, emitting[1:]):
        if t1 > 0 and 0 < len(truth[t1]) < cap < len(truth[t1]) + len(truth[t2]):
            return t1, t2
    return None


def save_ticks(truth):
    """(even tick, odd tick) at which to move the state into a fresh object: the even one directly follows an emitting tick, the odd one
    comes at least three ticks later."""
    even = next(t for t in range(6, len(truth), 2) if truth[t - 1])
    return even, even + 3


def rounding_gap(case, tr, gamma, eta):
    """(largest |priority(q rounded to float32) - priority(float64 q)| over the run's rows, largest priority): what keeping q in float32,
    as the window ring does, may move a priority by.  Host only."""
    exact, rounded = host_rows(case, tr, gamma, eta), host_rows(case, tr, gamma, eta, q_as=np.float32)
    gap = top = 0.0
    for out_e, out_r in zip(exact, rounded):
        assert [a for a, _ in out_e] == [a for a, _ in out_r]
        for (_, e), (_, r) in zip(out_e, out_r):
            gap, top = max(gap, abs(r["priority"].item() - e["priority"].item())), max(top, abs(e["priority"].item()))
    return gap, top


# ============================================================================= the case tables
# q_rounding_gap: rounding_gap() of the case, measured on the host (tests/test_r2d2_actors_cpu.py recomputes it) and rounded up to four
# digits; the kernel is allowed twice that, for the reason next to PRIORITY_TOL in tests/test_r2d2_actors_gpu.py: the ring keeps q in
# float32 and a priority combines two q values.
Case = namedtuple("Case", "group name N H S A seq burn n period pad ticks gamma eta seed schedule lo hi quiet q_scale rewards zero_q q_rounding_gap")


def _case(group, name, gap, N=3, H=8, S=5, A=3, seq=4, burn=1, n=3, period=2, pad=True, ticks=40, gamma=0.99, eta=0.9, seed=0, schedule="random", lo=None, hi=None,
          quiet=0, q_scale=3.0, rewards=(-1.0, 0.0, 0.5, 1.0), zero_q=0.0):
    L = seq + n
    lo = max(2, L // 2) if lo is None else lo   # episodes of about a window: ends at every phase of it, several within one window's time
    hi = L + n + 2 if hi is None else hi
    return Case(group, name, N, H, S, A, seq, burn, n, period, pad, ticks, gamma, eta, seed, schedule, lo, hi, quiet, q_scale, tuple(rewards), zero_q, gap)


def key(c):
    return (c.seq, c.burn, c.n, c.period, c.pad, c.S, c.A)


def tol(c):
    return 2.0 * c.q_rounding_gap


@functools.lru_cache(maxsize=None)
def built(c):
    """(trace, host rows) of a case: computed once per process and shared; callers leave both unchanged."""
    done = window_schedule(c.seq + c.n, c.n, c.ticks) if c.schedule == "window" else done_schedule(c.seed + 7, c.ticks, c.N, c.lo, c.hi, c.quiet)
    if c.group == "decisions":
        tr = decision_trace(c.seed, c.ticks, c.N, c.S, c.A, c.H, done)
    else:
        tr = trace(c.seed, c.ticks, c.N, c.S, c.A, c.H, done, c.q_scale, c.rewards, c.zero_q)
    return tr, host_rows(key(c), tr, c.gamma, c.eta)


def gap_of(c):
    return rounding_gap(key(c), built(c)[0], c.gamma, c.eta)


# case name -> q_rounding_gap, measured by rounding_gap() on the host (tests/test_r2d2_actors_cpu.py recomputes and prints every one)
GAPS = {
    "compact-N1-pad1": 1.497e-07,
    "compact-N1-pad0": 1.497e-07,
    "compact-N16-pad1": 4.397e-07,
    "compact-N16-pad0": 3.061e-07,
    "compact-N17-pad1": 3.317e-07,
    "compact-N17-pad0": 3.081e-07,
    "compact-N64-pad1": 5.562e-07,
    "compact-N64-pad0": 4.443e-07,
    "compact-N65-pad1": 4.256e-07,
    "compact-N65-pad0": 4.010e-07,
    "compact-N130-pad1": 6.156e-07,
    "compact-N130-pad0": 4.336e-07,
    "compact-N1024-pad1": 5.981e-07,
    "compact-N1024-pad0": 4.867e-07,
    "geom-seq128-burn40-n32-period0-pad1": 1.535e-07,
    "geom-seq128-burn40-n32-period0-pad0": 1.888e-07,
    "geom-seq128-burn40-n32-period1-pad1": 1.545e-07,
    "geom-seq128-burn40-n32-period1-pad0": 2.119e-07,
    "geom-seq128-burn40-n32-period150-pad1": 2.568e-07,
    "geom-seq128-burn40-n32-period150-pad0": 2.693e-07,
    "geom-seq128-burn40-n32-period167-pad1": 2.047e-07,
    "geom-seq128-burn40-n32-period167-pad0": 2.047e-07,
    "geom-seq159-burn158-n1-period0-pad1": 1.700e-07,
    "geom-seq159-burn158-n1-period0-pad0": 3.319e-08,
    "geom-seq159-burn158-n1-period1-pad1": 4.573e-07,
    "geom-seq159-burn158-n1-period1-pad0": 2.584e-07,
    "geom-seq159-burn158-n1-period150-pad1": 1.834e-07,
    "geom-seq159-burn158-n1-period150-pad0": 1.213e-07,
    "geom-seq159-burn158-n1-period167-pad1": 2.311e-07,
    "geom-seq159-burn158-n1-period167-pad0": 2.311e-07,
    "geom-seq1-burn0-n1-period0-pad1": 4.338e-07,
    "geom-seq1-burn0-n1-period0-pad0": 4.338e-07,
    "geom-seq1-burn0-n1-period1-pad1": 2.478e-07,
    "geom-seq1-burn0-n1-period1-pad0": 2.478e-07,
    "geom-seq1-burn0-n1-period2-pad1": 3.160e-07,
    "geom-seq1-burn0-n1-period2-pad0": 3.160e-07,
    "geom-seq1-burn0-n1-period9-pad1": 2.650e-07,
    "geom-seq1-burn0-n1-period9-pad0": 2.650e-07,
    "geom-seq155-burn0-n5-period0-pad1": 1.164e-07,
    "geom-seq155-burn0-n5-period0-pad0": 8.012e-08,
    "geom-seq155-burn0-n5-period1-pad1": 3.542e-07,
    "geom-seq155-burn0-n5-period1-pad0": 3.039e-07,
    "geom-seq155-burn0-n5-period150-pad1": 1.836e-07,
    "geom-seq155-burn0-n5-period150-pad0": 5.169e-07,
    "geom-seq155-burn0-n5-period167-pad1": 3.460e-07,
    "geom-seq155-burn0-n5-period167-pad0": 3.460e-07,
    "width-H4": 2.728e-07,
    "width-H68": 2.924e-07,
    "width-H1028": 2.230e-07,
    "width-S1": 2.317e-07,
    "width-S3": 2.020e-07,
    "width-S4": 2.345e-07,
    "width-S152": 2.382e-07,
    "width-A2": 2.813e-07,
    "width-A5": 4.289e-07,
    "width-A64": 2.130e-07,
    "width-S8-unaligned": 2.159e-07,
    "decide-A2": 4.118e-07,
    "decide-A64": 4.348e-07,
    "prio-q0.001-gamma0.997-eta0.9": 8.729e-11,
    "prio-q0.001-gamma1-eta0": 3.557e-11,
    "prio-q0.001-gamma0-eta1": 9.514e-11,
    "prio-q0.001-gamma0.99-eta0.5": 6.368e-11,
    "prio-q10-gamma0.997-eta0.9": 2.149e-06,
    "prio-q10-gamma1-eta0": 7.124e-07,
    "prio-q10-gamma0-eta1": 9.209e-07,
    "prio-q10-gamma0.99-eta0.5": 1.252e-06,
    "prio-q1000-gamma0.997-eta0.9": 9.771e-05,
    "prio-q1000-gamma1-eta0": 5.828e-05,
    "prio-q1000-gamma0-eta1": 1.029e-04,
    "prio-q1000-gamma0.99-eta0.5": 7.891e-05,
    "capacity-N5": 2.590e-07,
    "saveload": 2.601e-07,
}


def _table(group, specs):
    return tuple(_case(group, name, GAPS.get(name, float("nan")), **kw) for name, kw in specs)  # no recorded gap: every comparison fails


# --- compaction and grouping: one ballot with 1 lane, exactly one act group, one past it, a full ballot, one past it, a third partial
# ballot, the most actors accepted.  L = 5, episodes of 2..9 ticks after a first one of 5..12 that lets every actor fill its window.
_COMPACT = dict(seq=3, burn=1, n=2, period=2, S=5, A=3, H=4, lo=2, hi=9, quiet=3)
COMPACTION_SPECS = tuple((f"compact-N{N}-pad{int(pad)}", dict(_COMPACT, N=N, pad=pad, ticks=14 if N == 1024 else 24, seed=N))
                         for N in (1, 16, 17, 64, 65, 130, 1024) for pad in (True, False))

# --- window geometry: L = 160 (the LDS arrays' size), T = 1 at L = 160, L = 2, T = 155 lanes; store_period 0, 1, between, L + 7.
# The reference emits by period only at the tick at which store_period_stamp EQUALS store_period.  Without padding the stamp passes a period
# below L - 1 before the first window is full and never meets it again, unless the period is at least L / 2: the first emission, at tick
# L - 1, takes one period off and the stamp meets the period again at tick 2 * period.  The value between is L - L / 16 for that reason;
# with store_period 0 or 1 and no padding the host model emits only after an episode start (from a ring whose head has moved, not from one
# that has dropped records), and the tests hold the kernel to exactly that.
GEOMETRIES = ((128, 40, 32), (159, 158, 1), (1, 0, 1), (155, 0, 5))


def periods(L):
    return (0, 1, max(2, L - L // 16), L + 7)


GEOMETRY_SPECS = tuple((f"geom-seq{s}-burn{b}-n{n}-period{p}-pad{int(pad)}",
                        dict(seq=s, burn=b, n=n, period=p, pad=pad, ticks=2 * (s + n) + 20, seed=s + p, schedule="window" if s + n > 8 else "random", lo=2, hi=5))
                       for (s, b, n) in GEOMETRIES for p in periods(s + n) for pad in (True, False))

# --- copy widths: seq_len 4, n_step 3 (L = 7), one knob away from H = 8, S = 5, A = 3
WIDTH_SPECS = (tuple((f"width-H{H}", dict(H=H, seed=H)) for H in (4, 68, 1028)) + tuple((f"width-S{S}", dict(S=S, seed=S)) for S in (1, 3, 4, 152))
               + tuple((f"width-A{A}", dict(A=A, seed=A)) for A in (2, 5, 64)) + (("width-S8-unaligned", dict(S=8, seed=81)),))

# --- decisions
DECISION_SPECS = tuple((f"decide-A{A}", dict(N=33, A=A, H=4, ticks=12, seed=A, lo=2, hi=6)) for A in (2, 64))

# --- priority numerics: three |q| ranges x four (gamma, eta); q rows exactly zero in one of eight records.  1e3 stays: its measured gap
# is below 1e-7 of the priorities it is measured on (test_r2d2_actors_cpu.py asserts gap <= 1e-3 of that scale for every range)
PRIORITY_REWARDS = (-100.0, -1.0, 0.0, 0.5, 100.0)
PRIORITY_SPECS = tuple((f"prio-q{qs:g}-gamma{g:g}-eta{e:g}", dict(N=4, seq=6, burn=2, n=3, period=2, ticks=60, gamma=g, eta=e, q_scale=qs, rewards=PRIORITY_REWARDS,
                                                                 zero_q=0.125, seed=3, lo=2, hi=9))
                       for qs in (1e-3, 10.0, 1e3) for (g, e) in ((0.997, 0.9), (1.0, 0.0), (0.0, 1.0), (0.99, 0.5)))

# --- capacity and save / load: the first test's geometry family
CAPACITY_SPECS = (("capacity-N5", dict(N=5, seq=3, burn=1, n=2, period=2, ticks=20, seed=5, lo=2, hi=9)),)
SAVELOAD_SPECS = (("saveload", dict(period=2, ticks=40, seed=11, lo=3, hi=12)),)

COMPACTION, GEOMETRY, WIDTH = _table("compaction", COMPACTION_SPECS), _table("geometry", GEOMETRY_SPECS), _table("width", WIDTH_SPECS)
DECISIONS, PRIORITY = _table("decisions", DECISION_SPECS), _table("priority", PRIORITY_SPECS)
CAPACITY, SAVELOAD = _table("capacity", CAPACITY_SPECS), _table("saveload", SAVELOAD_SPECS)
ALL_CASES = COMPACTION + GEOMETRY + WIDTH + DECISIONS + PRIORITY + CAPACITY + SAVELOAD
