"""tests/store_model.py against the reference's replay ring (oracle.jorldy_oracle.ReplayOracle, which
tests/test_oracle_golden.py pins to the reference): the same random pushes, lengths of `capacity` and more
included, must leave the same index, counter and slot contents after every step, and the same sample under the
same global seed.  This pins the model before anything on the GPU is compared with it."""
import numpy as np
import pytest

import store_model as M
from oracle.jorldy_oracle import ReplayOracle

COLS = [("state", M.F32, 5), ("action", M.I64, 1), ("reward", M.F64, 1), ("frame", M.U8, 21), ("done", M.U8, 1), ("t", M.I32, 2)]


def _batch(rng, n, serial):
    """n rows per column; the push's serial number and the row number are written into the values."""
    out = {}
    for k, (nm, dt, elems) in enumerate(COLS):
        base = serial * 1000 + np.arange(n)[:, None] * 10 + k
        if dt == M.U8:
            out[nm] = ((base + np.arange(elems)[None, :] * 7) % 256).astype(np.uint8)
        elif dt in (M.F32, M.F64):
            out[nm] = (base + rng.rand(n, elems)).astype(M.NP_OF[dt])
        else:
            out[nm] = (base + rng.randint(0, 5, size=(n, elems))).astype(M.NP_OF[dt])
    return out


def _transitions(batch, n):
    return [{nm: batch[nm][j : j + 1] for nm, _, _ in COLS} for j in range(n)]


def _assert_same(model, ref, written):
    assert model.index == ref.buffer_index and model.counter == ref.buffer_counter and model.size == ref.size
    for s in range(model.capacity):
        t = ref.buffer[s]
        assert (t is not None) == written[s]
        for k, (nm, dt, elems) in enumerate(COLS):
            if t is None:  # never written: still the sentinel
                np.testing.assert_array_equal(model.cols[nm][s], M.sentinel(model.capacity, elems, M.NP_OF[dt], salt=k)[s])
            else:
                assert model.cols[nm].dtype == t[nm].dtype
                np.testing.assert_array_equal(model.cols[nm][s], t[nm][0])


@pytest.mark.parametrize("capacity,seed", [(1, 0), (7, 1), (16, 2), (37, 3)])
def test_model_ring_is_the_reference_ring(capacity, seed):
    rng = np.random.RandomState(seed)
    model, ref = M.StoreModel(capacity, COLS), ReplayOracle(capacity)
    written = np.zeros(capacity, dtype=bool)
    lengths = [1, capacity, capacity + 1, 2 * capacity + 3, 3 * capacity] + [int(x) for x in rng.randint(1, 3 * capacity + 2, size=40)]
    rng.shuffle(lengths)
    for serial, n in enumerate(lengths):
        b = _batch(rng, n, serial)
        written[(model.index + np.arange(n)) % capacity] = True
        assert model.push(b) == n
        ref.store(_transitions(b, n))
        _assert_same(model, ref, written)
        # the same global seed on both sides: replay_buffer.py:26 draws np.random.randint(counter, size=B)
        B = 1 + serial % 9
        np.random.seed(100 + serial)
        want = ref.sample(B)
        np.random.seed(100 + serial)
        got = model.gather(np.random.randint(model.counter, size=B), as_float=False)
        as_f = model.gather(np.random.RandomState(100 + serial).randint(model.counter, size=B))
        for nm, _, _ in COLS:
            np.testing.assert_array_equal(got[nm], want[nm])
            assert got[nm].dtype == want[nm].dtype and as_f[nm].dtype == np.float32
            np.testing.assert_array_equal(as_f[nm], want[nm].astype(np.float32))


def test_model_push_prefix_of_a_longer_source():
    """push(cols, n) takes the first n rows of a longer source, as ops.DeviceStore.push_device does."""
    rng = np.random.RandomState(5)
    a, b = M.StoreModel(9, COLS), M.StoreModel(9, COLS)
    for serial, n in enumerate([4, 9, 2, 7]):
        src = _batch(rng, 11, serial)
        a.push(src, n)
        b.push({nm: v[:n] for nm, v in src.items()})
        assert (a.index, a.counter) == (b.index, b.counter)
        for nm in a.names:
            np.testing.assert_array_equal(a.cols[nm], b.cols[nm])


def test_model_write_rows_skips_bad_slots_and_keeps_the_ring_position():
    rng = np.random.RandomState(6)
    m = M.StoreModel(12, COLS)
    m.push(_batch(rng, 5, 0))
    before = {nm: m.cols[nm].copy() for nm in m.names}
    rows = _batch(rng, 6, 1)
    slots = np.array([3, -1, 11, 12, 2**40, 0])
    m.write_rows(slots, rows)
    assert (m.index, m.counter) == (5, 5)
    for nm in m.names:
        want = before[nm].copy()
        for i, s in enumerate(slots):
            if 0 <= s < 12:
                want[s] = rows[nm][i]
        np.testing.assert_array_equal(m.cols[nm], want)
    m.write_rows(np.zeros(0, dtype=np.int64), _batch(rng, 0, 2))
    m.clear()
    assert (m.index, m.counter) == (0, 0)


def test_model_gather_clamps_and_rounds_to_nearest_even():
    m = M.StoreModel(37, [("a", M.I64, 1), ("d", M.F64, 1)])
    a = np.arange(37, dtype=np.int64)[:, None].copy()
    a[:3, 0] = [2**24 + 1, -(2**53) - 1, 2**62]
    d = np.arange(37, dtype=np.float64)[:, None] + 0.5
    d[:3, 0] = [1 + 2.0**-30, 1e300, -0.0]
    m.push({"a": a, "d": d})
    g = m.gather([999, 1000, 1036, 1037], idx_offset=1000)
    np.testing.assert_array_equal(g["a"][:, 0], np.array([2**24, 2**24, 36, 36], dtype=np.float32))  # 2**24 + 1 is a tie: to even
    h = m.gather([0, 1, 2], as_float={"a": False})
    assert h["a"].dtype == np.int64 and h["d"].dtype == np.float32
    np.testing.assert_array_equal(h["a"][:, 0], a[:3, 0])
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(h["d"][:, 0].view(np.uint32), np.array([1.0, np.inf, -0.0], dtype=np.float32).view(np.uint32))
