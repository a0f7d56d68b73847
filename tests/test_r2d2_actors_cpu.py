"""The batched R2D2 actors' host model without a GPU (tests/r2d2_actors_truth.py): every recorded priority tolerance is measured again, decide()
is held to hand-written examples, and every schedule is shown to reach the kernel branch its GPU case is there for, from the host rows alone."""
import numpy as np
import pytest

import r2d2_actors_truth as T

IDS = [c.name for c in T.ALL_CASES]


@pytest.mark.parametrize("c", T.ALL_CASES, ids=IDS)
def test_recorded_q_rounding_gap_is_the_measured_one(c):
    """host_rows(q_as=float32) against host_rows(): the recorded gap covers the measured one, is not looser than its rounding to four
    digits, and is nonzero (every case keeps float64 q that float32 cannot hold; an exact 0 would make the GPU tolerance 0)."""
    gap, top = T.gap_of(c)
    print(f"{c.name}: measured q rounding gap {gap:.4e} (recorded {c.q_rounding_gap:.4e}), largest priority {top:.3e}")
    assert 0.0 < gap <= c.q_rounding_gap <= 1.001 * gap


@pytest.mark.parametrize("c", T.PRIORITY, ids=[c.name for c in T.PRIORITY])
def test_priority_tolerance_cannot_hide_a_wrong_fold(c):
    """The allowed gap is below 1e-3 of the case's mean priority (|q| about 1e3 stays in: 2e-4 against priorities of 1e3); exact zeros are
    among the q values taken."""
    tr, truth = T.built(c)
    prios = [r["priority"].item() for out in truth for _, r in out]
    taken = np.take_along_axis(tr["q"], tr["action"][..., None], -1)
    assert T.tol(c) <= 1e-3 * np.mean(prios) and (taken == 0.0).sum() >= 10 and len(prios) >= 100


def test_decide_examples():
    f = lambda *rows: np.asarray(rows, dtype=np.float32)
    act, qt = T.decide(f([1.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0], [-1.0, -2.0, -0.5, -0.5]), None, None, None)
    assert act.tolist() == [1, 0, 2] and qt.tolist() == [3.0, 0.0, -0.5], "a tie: the first maximum"
    act, qt = T.decide(f([1.0, 2.0, 2.5], [-3.0, -2.0, -1.0]), None, None, None)
    assert act.tolist() == [2, 2] and qt.tolist() == [2.5, -1.0], "the maximum at A - 1"
    eps = np.asarray([0.3, 0.3, 0.3, 0.7, 0.7], np.float32)
    e = eps.astype(np.float64)
    q = f(*([[5.0, 1.0, 2.0]] * 5))
    ra = np.asarray([2, 2, 2, 2, 2])
    # u == eps: greedy (strict <); the float64 just below: random; the decimal 0.3 is below float32(0.3): random, 0.7 is above float32(0.7): greedy
    act, qt = T.decide(q, eps, np.asarray([e[0], np.nextafter(e[1], 0.0), 0.3, 0.7, np.nextafter(e[4], 1.0)]), ra)
    assert e[0] > 0.3 and e[3] < 0.7
    assert act.tolist() == [0, 2, 2, 0, 0] and qt.tolist() == [5.0, 2.0, 2.0, 5.0, 5.0]
    act, qt = T.decide(f([5.0, 1.0, 2.0], [1.0, 5.0, 2.0], [1.0, 5.0, 2.0]), np.ones(3, np.float32), np.zeros(3), np.asarray([-1, 3, 7]))
    assert act.tolist() == [0, 2, 2] and qt.tolist() == [5.0, 2.0, 2.0], "rand_action = -1 and = A (and beyond) are clamped"
    assert act.dtype == np.int64 and qt.dtype == np.float32


def test_moved_helpers_reproduce_the_first_tests_schedule_and_tolerance():
    """tests/test_r2d2_actors_gpu.py's cases through the moved helpers: a full window everywhere and a short one with padding (its own
    assertion), and the 4.96e-7 its PRIORITY_TOL was measured as."""
    import test_r2d2_actors_gpu as G

    worst = 0.0
    for case in G.CASES:
        seq, burn, n, period, pad, S, A = case
        tr = T.trace(seq * 100 + n, G.TICKS, G.N, S, A, G.H, T.done_from_sets(G.DONES, G.TICKS))
        lens = T.window_lengths(T.host_rows(case, tr, G.GAMMA, G.ETA))
        assert seq + n in lens and (not pad or min(lens) < seq + n), "the schedule yields a full window and, with padding, a short one"
        worst = max(worst, T.rounding_gap(case, tr, G.GAMMA, G.ETA)[0])
    assert 4.95e-7 < worst <= 4.96e-7 and G.PRIORITY_TOL == 2 * 4.96e-7


def _emitters(c):
    """[ticks, N] bool: who emits when."""
    _, truth = T.built(c)
    e = np.zeros((c.ticks, c.N), bool)
    for t, out in enumerate(truth):
        e[t, [a for a, _ in out]] = True
    return e


@pytest.mark.parametrize("c", T.COMPACTION, ids=[c.name for c in T.COMPACTION])
def test_compaction_schedules_reach_every_ballot(c):
    """With N >= 130: a tick on which every 64-actor block holds an emitter and a non-emitter; one on which an actor from 128 up has some,
    not all, of the actors below it emitting; one without any emitter; one on which all emit.  Every N: rows pile up over several ticks
    between two restarts, within the 8 * N rows of the output."""
    e = _emitters(c)
    held = [int(e[t0:t0 + 8].sum()) for t0 in range(0, c.ticks, 8)]
    assert max(held) <= 8 * c.N and e.any(1).sum() >= (4 if c.N >= 16 else 3) and T.built(c)[0]["done"].sum() >= 3
    if c.N < 130:
        return
    blocks = [slice(b, min(b + 64, c.N)) for b in range(0, c.N, 64)]
    assert any(all(e[t, b].any() and not e[t, b].all() for b in blocks) for t in range(c.ticks)), "mixed in every block of 64"
    below = np.cumsum(e, axis=1) - e  # emitters below actor a
    a = np.arange(c.N)
    assert ((below > 0) & (below < a) & (a >= 128))[e.any(1)].any(), "a partial prefix above two full ballots"
    assert (~e.any(1)).any() and e.all(1).any(), "a tick without emitters and a tick on which every actor emits"
    assert len({int(col.argmax()) for col in T.built(c)[0]["done"].T if col.any()}) >= 6, "the actors are out of phase"
    assert sum(all(e[t, b].any() and not e[t, b].all() for b in blocks) for t in range(c.ticks)) >= 2


@pytest.mark.parametrize("c", T.GEOMETRY, ids=[c.name for c in T.GEOMETRY])
def test_geometry_schedules_wrap_the_ring_and_pad_windows(c):
    """Several episode ends and emitted rows in every case.  Without padding: an emission from a window that has dropped records (more than
    L appended since its last cut) wherever the reference can emit one -- store_period >= L / 2, see the case table; L = 2 also at 1 -- and
    otherwise an emission after a cut, from a ring whose head is not 0.  With padding (and L > n_step + 1, so that a short window
    exists): a short window in every case, a full one wherever the reference emits by period."""
    tr, truth = T.built(c)
    L = c.seq + c.n
    ages = []
    T.host_rows(T.key(c), tr, c.gamma, c.eta, ages=ages)
    lens = T.window_lengths(truth)
    assert c.ticks >= 2 * L + 20 and tr["done"].sum() >= 3 and len(lens) >= 3 and len(lens) == len(ages)
    by_period = c.period >= L / 2 and (L > 8 or c.period <= L)
    if not c.pad:
        assert set(lens) == {L}
        if by_period or (L == 2 and c.period == 1):
            assert any(age > L for _, _, age in ages), "an emission after the ring has wrapped"
        assert any(t >= L and age <= t for t, _, age in ages), "an emission after a cut"
    elif L > c.n + 1:
        assert min(lens) < L, "a short window"
        if by_period:
            assert L in lens and any(age > L for _, _, age in ages), "a full window, after the ring has wrapped"


def test_geometry_table_is_what_the_kernel_limits_ask_for():
    geoms = {(c.seq, c.burn, c.n) for c in T.GEOMETRY}
    assert geoms == {(128, 40, 32), (159, 158, 1), (1, 0, 1), (155, 0, 5)} and max(s + n for s, _, n in geoms) == 160
    for g in geoms:
        L = g[0] + g[2]
        for pad in (True, False):
            got = sorted(c.period for c in T.GEOMETRY if (c.seq, c.burn, c.n) == g and c.pad == pad)
            assert got[0] == 0 and got[1] == 1 and 1 < got[2] <= L and got[3] == L + 7 and len(got) == 4
    assert all(c.N == 3 for c in T.GEOMETRY)


@pytest.mark.parametrize("c", T.PRIORITY, ids=[c.name for c in T.PRIORITY])
def test_priority_schedule_puts_a_done_at_every_fold_position(c):
    """Fold position i of trained step t reads done[i + n_burn_in + t] of the stored row: every i in 0..n_step-1 sees a done in some row,
    at the first and at the last trained step too; full and short windows both occur."""
    _, truth = T.built(c)
    T_, seen = c.seq - c.burn, set()
    for out in truth:
        for _, r in out:
            d = r["done"][0, :, 0]
            seen |= {(i, t) for i in range(c.n) for t in range(T_) if d[i + c.burn + t]}
    assert {i for i, _ in seen} == set(range(c.n))
    assert {(i, T_ - 1) for i in range(c.n)} <= seen and len({t for _, t in seen}) > 1  # a window is cut n_step ticks after a done: none lies deeper
    lens = T.window_lengths(truth)
    assert c.seq + c.n in lens and min(lens) < c.seq + c.n
    assert {(c.gamma, c.eta) for c in T.PRIORITY} == {(0.997, 0.9), (1.0, 0.0), (0.0, 1.0), (0.99, 0.5)}


@pytest.mark.parametrize("c", T.DECISIONS, ids=[c.name for c in T.DECISIONS])
def test_decision_trace_holds_every_kind_of_tick_and_draw(c):
    tr, truth = T.built(c)
    kinds = ["greedy" if tr["eps"][t] is None else "forced" if (tr["eps"][t] == 1).all() else "mixed" for t in range(c.ticks)]
    assert min(kinds.count(k) for k in ("greedy", "mixed", "forced")) >= 3
    for t in (t for t, k in enumerate(kinds) if k == "mixed"):
        q32, e, u, ra = tr["q"][t].astype(np.float32), tr["eps"][t].astype(np.float64), tr["u"][t], tr["rand"][t]
        assert (u < e).any() and (u == e).any() and (u > e).any() and (ra == -1).any() and (ra == c.A).any()
        rnd = u < e
        assert (rnd & (ra == -1)).any() and (rnd & (ra == c.A)).any(), "a clamped draw is taken"
        top = q32.max(-1, keepdims=True)
        assert ((q32 == top).sum(-1) >= 2).any() and (q32.argmax(-1) == c.A - 1).any(), "ties and a maximum at A - 1"
        greedy = ~rnd
        assert (greedy & ((q32 == top).sum(-1) >= 2)).any() and (tr["action"][t][greedy] == q32.argmax(-1)[greedy]).all()
    assert c.N == 33 and c.ticks == 12 and sum(len(o) for o in truth) > 0
    after = tr["done"][:-1]
    assert after.any() and not tr["h"][1:][after].any() and not tr["c"][1:][after].any() and (tr["h"][1:][~after] == tr["hn"][:-1][~after]).all()


def test_capacity_case_overflows_in_the_middle_of_a_tick():
    c = T.CAPACITY[0]
    _, truth = T.built(c)
    t1, t2 = T.overflow_ticks(truth, c.N)
    assert all(not truth[t] for t in range(t1 + 1, t2)) and 0 < len(truth[t1]) < c.N < len(truth[t1]) + len(truth[t2])
    assert sum(len(truth[t]) for t in range(t2 + 1, c.ticks)) >= c.N, "rows after the overflow show that the state machines went on"


def test_save_load_ticks_are_one_even_one_odd_and_one_follows_an_emission():
    c = T.SAVELOAD[0]
    _, truth = T.built(c)
    even, odd = T.save_ticks(truth)
    assert even % 2 == 0 and odd % 2 == 1 and truth[even - 1] and even < odd < c.ticks - 8
    assert sum(len(truth[t]) for t in range(odd, c.ticks)) >= 5
