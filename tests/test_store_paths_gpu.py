"""ops.DeviceStore (jh_store.hip) against the numpy ring model of tests/store_model.py, bit for bit.

Every step compares every WHOLE column as bytes, and index / size, with the model: the columns start from the
model's sentinel pattern, so a row that never arrived and a write that landed outside its rows both fail the step
that made them.  Row values are random bytes (uint8) or random finite numbers: a 16-byte piece that was shifted,
duplicated or carried over from another push does not compare equal.  There is no tolerance in this file.

Branches of jh_store.hip reached (sizes are the smallest that reach them):
  jh_store_copy_cols_kernel   16-byte path / scalar fallback / scalar tail / the split at the wrap at aligned and
                              unaligned `first` (a); the 2048-block cap with a second grid-stride round (b)
  copy-engine commit          > 512 KB of rows (c), > 8 columns (e); jh_store_append for push_device of > 8 columns (e)
  jh_store_push, n > capacity (d)
  jh_scatter_rows_kernel      row_bytes % 16 == 0 and != 0, bad slots, gx at its cap of 64, the wrapper's chunks (f)
  jh_gather_kernel            every source type to itself and to float32, idx_offset and its clamp, both grid caps,
                              n_sel == 16, mixed as_float, out= (e, g)
"""
import numpy as np
import pytest

from store_model import F32, F64, I32, I64, U8, StoreModel
from tests.util import cu, npy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch

    assert torch.cuda.is_available()
    from jorldy_amd import _lib as L
    from jorldy_amd import ops as _ops

    assert (L.JH_U8, L.JH_F32, L.JH_I64, L.JH_F64, L.JH_I32) == (U8, F32, I64, F64, I32)
    return _ops


# ----------------------------------------------------------------------------- helpers
def _make(ops, capacity, cols):
    """(DeviceStore, StoreModel) holding the same bytes: the device columns start from the model's sentinel."""
    import torch

    st = ops.DeviceStore(capacity, [(nm, dt, e, (e,)) for nm, dt, e in cols])
    m = StoreModel(capacity, cols)
    for nm in m.names:
        st.column(nm).copy_(torch.from_numpy(m.cols[nm]))
    _check(st, m)
    return st, m


def _check(st, m, what=""):
    import torch

    torch.cuda.synchronize()
    assert (st.index, st.size) == (m.index, m.size), what
    for nm in m.names:
        got = npy(st.column(nm))
        assert got.dtype == m.cols[nm].dtype and got.shape == m.cols[nm].shape
        np.testing.assert_array_equal(got.view(np.uint8), m.cols[nm].view(np.uint8), err_msg=f"column {nm} {what}")


def _rows(rng, m, n, tag=None):
    """n random rows per column; tag=True writes the column's number into the values (a swapped pointer shows)."""
    out = {}
    for k, nm in enumerate(m.names):
        e, dt = m.elems[nm], m.dtype[nm]
        if dt == np.uint8:
            v = rng.randint(0, 256, size=(n, e))
        elif dt == np.float32:
            v = rng.standard_normal((n, e)) * 1e3
        elif dt == np.float64:
            v = rng.standard_normal((n, e)) * 1e6
        elif dt == np.int64:
            v = rng.randint(-(2**62), 2**62, size=(n, e), dtype=np.int64)
        else:
            v = rng.randint(-(2**31), 2**31, size=(n, e), dtype=np.int64)
        if tag:
            v = np.floor(v) % 1000 + 1000 * k
        out[nm] = np.ascontiguousarray(v.astype(dt))
    return out


def _append(st, m, rows, n, mode):
    """The same n rows into the store (by `mode`) and into the model."""
    if mode == "push":
        assert st.push(rows) == n
    elif mode == "stage":
        views = st.stage(n)
        for nm in m.names:
            assert views[nm].shape == (n, m.elems[nm]) and views[nm].dtype == m.dtype[nm]
            views[nm][:] = rows[nm]
        st.commit()
    else:
        st.push_device({nm: cu(rows[nm]) for nm in m.names}, n)
    m.push(rows)


def _assert_gather(st, m, idx, **kw):
    """gather(**kw) on the device == the model's, in dtype, shape and bits."""
    got = st.gather(cu(np.asarray(idx, dtype=np.int64)), **kw)
    want = m.gather(idx, idx_offset=kw.get("idx_offset", 0), names=kw.get("names"), as_float=kw.get("as_float", True))
    assert list(got.keys()) == list(want.keys())
    for nm in want:
        g = npy(got[nm])
        assert g.dtype == want[nm].dtype and g.shape == want[nm].shape, nm
        np.testing.assert_array_equal(g.view(np.uint8), want[nm].view(np.uint8), err_msg=f"gather {nm}")
    return got


# ----------------------------------------------------------------------------- (a) one-launch append
A_COLS = [("f", F32, 5), ("b", U8, 1), ("img", U8, 105), ("v", F32, 4), ("a", I64, 1), ("d", F64, 3), ("i", I32, 7)]
A_CAP = 37
# index before each push: 0 1 4 20 0 36 36 4 21 15 17 17 0 0 33 17 12
A_LENGTHS = [1, 3, 16, 17, 36, 37, 5, 17, 31, 2, 37, 20, 37, 33, 21, 32, 36]


def test_append_lengths_reach_what_they_are_chosen_for():
    """The fixed lengths of (a): >= 4 wraps; a wrap with `first * row_bytes` a multiple of 16 and one without, for one
    column; an aligned no-wrap append for the 20-byte rows (the 16-byte path) and an unaligned one; a push that
    exactly fills the ring; pushes that start at index 0."""
    rb = {nm: e * np.dtype({U8: "u1", F32: "f4", I64: "i8", F64: "f8", I32: "i4"}[dt]).itemsize for nm, dt, e in A_COLS}
    index, wraps, starts = 0, [], []
    vec_nowrap = {nm: set() for nm in rb}
    for n in A_LENGTHS:
        first = min(A_CAP - index, n)
        starts.append(index)
        if first < n:
            wraps.append(first)
        else:
            for nm in rb:
                vec_nowrap[nm].add((rb[nm] * index) % 16 == 0 and (rb[nm] * n) % 16 == 0)
        index = (index + n) % A_CAP
    assert len(wraps) >= 4 and A_CAP in A_LENGTHS and starts.count(0) >= 3
    for nm in ("b", "a", "f", "img"):
        assert {(f * rb[nm]) % 16 == 0 for f in wraps} == {True, False}, nm
    assert vec_nowrap["f"] == {True, False} and vec_nowrap["v"] == {True}


@pytest.mark.parametrize("mode", ["push", "stage", "push_device"])
def test_append_every_alignment(ops, mode):
    rng = np.random.RandomState(11)
    st, m = _make(ops, A_CAP, A_COLS)
    for step, n in enumerate(A_LENGTHS):
        _append(st, m, _rows(rng, m, n), n, mode)
        _check(st, m, f"after {mode} #{step} of {n} rows")


@pytest.mark.parametrize("mode", ["push", "stage", "push_device"])
def test_append_vector_part_then_scalar_tail(ops, mode):
    """The 16-byte path needs ring position, column base and `first` aligned, so an append that does not wrap has no
    tail (first == total) and capacity 37 never takes the path with rows that are no multiple of 16 bytes.  Capacity
    16, index 12, 7 rows: 8-byte rows give 32 bytes before the wrap and 56 in all (three pieces, 8 bytes of tail),
    12-byte rows 48 and 84 (five pieces, 4 bytes of tail); the 5-byte rows start unaligned (scalar fallback)."""
    rng = np.random.RandomState(25)
    st, m = _make(ops, 16, [("a", I64, 1), ("s", F32, 3), ("k", U8, 5)])
    for n in (12, 7, 9, 5):  # index 12 -> 3 -> 12 -> 1: the second wrap has 32 + 8 and 48 + 12 bytes
        _append(st, m, _rows(rng, m, n), n, mode)
        _check(st, m, f"after {mode} of {n} rows")


# ----------------------------------------------------------------------------- (b) grid cap
@pytest.fixture(scope="module")
def wide(ops):
    """("x", U8, 4096) x 2400 after the appends of (b); test_gather_grid_cap_vector_path reads it."""
    rng = np.random.RandomState(12)
    st, m = _make(ops, 2400, [("x", U8, 4096)])
    _append(st, m, _rows(rng, m, 200), 200, "push_device")
    _check(st, m, "200 rows")
    # 9.4 MB: 2300 blocks' worth of 16-byte pieces on a grid capped at 2048 -> a second grid-stride round, and a wrap
    _append(st, m, _rows(rng, m, 2300), 2300, "push_device")
    _check(st, m, "2300 rows from index 200")
    st.clear()
    m.clear()
    _append(st, m, _rows(rng, m, 2049), 2049, "push_device")
    _check(st, m, "2049 rows from index 0")
    return st, m


def test_append_grid_cap(wide):
    st, m = wide
    assert (st.index, st.size) == (2049, 2049)


# ----------------------------------------------------------------------------- (c) copy-engine commit
def test_commit_above_the_one_launch_limit(ops):
    rng = np.random.RandomState(13)
    st, m = _make(ops, 40, [("state", U8, 28224), ("r", F32, 1)])
    for n in (24, 24, 1):  # 677 KB (> 512 KB: two copies per column around the wrap), again across the wrap, then the kernel form
        _append(st, m, _rows(rng, m, n), n, "push")
        _check(st, m, f"after {n} rows")
    assert st.index == 9


# ----------------------------------------------------------------------------- (d) longer than the ring
def test_push_longer_than_the_ring(ops):
    rng = np.random.RandomState(14)
    st, m = _make(ops, 16, [("s", F32, 3), ("k", U8, 5), ("a", I64, 1)])
    _append(st, m, _rows(rng, m, 5), 5, "push")
    for n in (16, 17, 40, 33):
        assert st.index != 0
        _append(st, m, _rows(rng, m, n), n, "push")
        _check(st, m, f"after {n} rows")


# ----------------------------------------------------------------------------- (e) column counts
@pytest.mark.parametrize("n_cols", [1, 8, 9, 14, 15, 16])
def test_column_counts(ops, n_cols):
    """<= 8 columns: one launch for push / commit / push_device; more: a copy per column (jh_store_append for
    push_device).  jh_store_create takes up to 16 columns, so all of them must be pushable."""
    rng = np.random.RandomState(15)
    st, m = _make(ops, 11, [(f"c{k}", F32, 3) for k in range(n_cols)])
    for mode, n in (("push", 7), ("push", 7), ("stage", 6), ("push_device", 5), ("push_device", 9), ("stage", 11), ("push", 26)):
        _append(st, m, _rows(rng, m, n, tag=True), n, mode)
        _check(st, m, f"{n_cols} columns after {mode} of {n}")
    idx = rng.permutation(11)
    _assert_gather(st, m, idx)  # n_sel == n_cols
    _assert_gather(st, m, idx, names=m.names[::-1], as_float=False)


# ----------------------------------------------------------------------------- (f) write_rows
F_COLS = [("p", U8, 105), ("q", U8, 4096 * 5), ("w", F32, 4)]


def _scatter(st, m, slots, rows):
    before = (st.index, st.size)
    st.write_rows(slots, rows)
    m.write_rows(slots, rows)
    _check(st, m, f"write_rows of {len(slots)}")
    assert (st.index, st.size) == before


@pytest.fixture(scope="module")
def pool(ops):
    """The store of (f) after its positional writes; the mixed gather of (g) reads it."""
    rng = np.random.RandomState(16)
    st, m = _make(ops, 50, F_COLS)
    _append(st, m, _rows(rng, m, 20), 20, "push")
    _scatter(st, m, rng.permutation(50)[:23], _rows(rng, m, 23))
    # slots outside [0, capacity) are skipped; their neighbours (49, 0 and the rows beside them in the call) stay intact
    slots = np.array([49, -1, 0, 50, 7, 2**40, 31, -(2**40), 51], dtype=np.int64)
    _scatter(st, m, slots, _rows(rng, m, slots.size))
    _scatter(st, m, np.zeros(0, dtype=np.int64), _rows(rng, m, 0))
    _scatter(st, m, rng.permutation(50), _rows(rng, m, 50))
    return st, m


def test_write_rows(pool):
    st, m = pool
    assert (st.index, st.size) == (20, 20)


def test_write_rows_wider_than_the_grid(ops):
    """gx = ceil(row_bytes / 4096) is capped at 64: a row of more than 256 KB takes a second grid-stride round."""
    rng = np.random.RandomState(17)
    st, m = _make(ops, 3, [("big", U8, 64 * 4096 + 48)])
    _scatter(st, m, np.array([2, 0]), _rows(rng, m, 2))
    _scatter(st, m, np.array([3, 1, -1]), _rows(rng, m, 3))


@pytest.fixture(scope="module")
def narrow(ops):
    """("w", F32, 1) x 70000 after one write_rows call of 40000 rows (the wrapper cuts it at 32768)."""
    rng = np.random.RandomState(18)
    st, m = _make(ops, 70000, [("w", F32, 1)])
    _scatter(st, m, rng.permutation(70000)[:40000], _rows(rng, m, 40000))
    return st, m


def test_write_rows_chunks(narrow):
    st, m = narrow
    assert (st.index, st.size) == (0, 0)


# ----------------------------------------------------------------------------- (g) gather
@pytest.fixture(scope="module")
def filled(ops):
    """The store of (a) after its pushes, then one full ring whose first rows hold the values float32 cannot hold."""
    rng = np.random.RandomState(19)
    st, m = _make(ops, A_CAP, A_COLS)
    for n in A_LENGTHS:
        _append(st, m, _rows(rng, m, n), n, "push")
    st.clear()
    m.clear()
    rows = _rows(rng, m, A_CAP)
    rows["a"][:3, 0] = [2**24 + 1, -(2**53) - 1, 2**62]
    rows["d"][0] = [1 + 2.0**-30, 1e300, -0.0]
    rows["d"][1] = [-1e300, 2.0**-150, 16777217.0]  # -inf, below float32's subnormals, a tie
    rows["d"][2, 0] = 2.0**-140  # a float32 subnormal
    rows["i"][0, :3] = [2**24 + 1, -(2**31), 2**31 - 1]
    _append(st, m, rows, A_CAP, "push")
    _check(st, m)
    return st, m


@pytest.mark.parametrize("as_float", [True, False, {"img": False, "a": False, "d": True, "i": False, "b": True}])
def test_gather_types(filled, as_float):
    st, m = filled
    rng = np.random.RandomState(20)
    idx = np.concatenate([np.arange(A_CAP), rng.randint(0, A_CAP, size=64)])
    _assert_gather(st, m, idx, as_float=as_float)
    _assert_gather(st, m, idx, as_float=as_float, names=["d", "img", "a", "f", "b", "i", "v"])
    for nm in m.names:
        _assert_gather(st, m, idx[:5], as_float=as_float, names=[nm])


def test_gather_values_float32_cannot_hold(filled):
    st, m = filled
    got = st.gather(cu(np.arange(3)), names=["a", "d", "i"])
    a = np.array([2**24 + 1, -(2**53) - 1, 2**62], dtype=np.int64)
    np.testing.assert_array_equal(npy(got["a"])[:, 0], a.astype(np.float32))
    assert npy(got["a"])[0, 0] == 2.0**24 and npy(got["a"])[1, 0] == -(2.0**53)  # ties go to even
    d = np.array([[1 + 2.0**-30, 1e300, -0.0], [-1e300, 2.0**-150, 16777217.0]])
    with np.errstate(over="ignore", under="ignore"):
        want = d.astype(np.float32)
    np.testing.assert_array_equal(npy(got["d"])[:2].view(np.uint32), want.view(np.uint32))
    assert want[0, 2] == 0 and np.signbit(want[0, 2]) and np.isinf(want[0, 1]) and want[1, 1] == 0 and want[1, 2] == 16777216.0
    np.testing.assert_array_equal(npy(got["i"])[0, :3], np.array([2**24 + 1, -(2**31), 2**31 - 1], dtype=np.int32).astype(np.float32))
    raw = st.gather(cu(np.arange(3)), names=["a", "d"], as_float=False)
    np.testing.assert_array_equal(npy(raw["a"])[:, 0], a)
    np.testing.assert_array_equal(npy(raw["d"])[:2].view(np.uint64), d.view(np.uint64))


def test_gather_idx_offset_and_clamp(filled):
    st, m = filled
    idx = np.array([999, 1000, 1036, 1037, 1018, 0, 2**40, -(2**40)])
    got = _assert_gather(st, m, idx, idx_offset=1000, as_float=False)
    np.testing.assert_array_equal(npy(got["i"]), m.cols["i"][[0, 0, 36, 36, 18, 0, 36, 0]])
    _assert_gather(st, m, idx, idx_offset=1000)
    _assert_gather(st, m, np.array([-5, 0, 36, 37, 12]))
    _assert_gather(st, m, np.array([3, 4, 40]), idx_offset=-2, names=["img", "a"])


def test_gather_one_row_and_none(filled):
    import torch

    st, m = filled
    _assert_gather(st, m, np.array([36]))
    _assert_gather(st, m, np.array([0]), as_float=False)
    for kw in ({}, {"as_float": False}):
        got = st.gather(torch.empty(0, dtype=torch.int64, device="cuda"), **kw)
        want = m.gather(np.zeros(0, dtype=np.int64), **kw)
        for nm in m.names:
            assert tuple(got[nm].shape) == want[nm].shape == (0, m.elems[nm]) and npy(got[nm]).dtype == want[nm].dtype
    _check(st, m)


def test_gather_static_out_buffers(filled):
    import torch

    st, m = filled
    as_float = {"img": False, "a": False}
    names = ["img", "f", "a", "d"]
    out = {nm: torch.full((9, m.elems[nm]), 7, dtype=torch.float32 if as_float.get(nm, True) else {"img": torch.uint8, "a": torch.int64}[nm], device="cuda")
           for nm in names}
    for idx in (np.array([0, 5, 36, 36, 1, 2, 3, 4, 9]), np.array([8, 7, 6, 5, 4, 3, 2, 1, 30])):
        got = st.gather(cu(idx), names=names, as_float=as_float, out=out)
        want = m.gather(idx, names=names, as_float=as_float)
        for nm in names:
            assert got[nm] is out[nm]
            np.testing.assert_array_equal(npy(out[nm]).view(np.uint8), want[nm].view(np.uint8))


def test_gather_grid_cap_generic_path(filled, narrow):
    rng = np.random.RandomState(21)
    st, m = filled
    _assert_gather(st, m, rng.randint(0, A_CAP, size=6000))  # img: 630000 elements = 2461 blocks' worth on 2048
    _assert_gather(st, m, rng.randint(0, A_CAP, size=6000), as_float=False, names=["img", "d"])
    st, m = narrow
    _assert_gather(st, m, rng.randint(0, 70000, size=70000))
    _assert_gather(st, m, rng.randint(0, 70000, size=70000) + 5, idx_offset=5, as_float=False)


def test_gather_grid_cap_vector_path(wide):
    rng = np.random.RandomState(22)
    st, m = wide
    idx = rng.randint(0, 2400, size=3000)  # 768000 16-byte pieces = 3000 blocks' worth on 2048
    _assert_gather(st, m, idx, as_float=False)
    _assert_gather(st, m, idx)
    _assert_gather(st, m, idx + 77, idx_offset=77, as_float=False)


def test_gather_mixed_vector_and_generic_in_one_launch(pool):
    rng = np.random.RandomState(23)
    st, m = pool
    idx = rng.randint(0, 50, size=33)
    for as_float in ({"p": False, "q": True, "w": True}, {"p": True, "q": False}, {"q": False, "p": False, "w": False}):
        _assert_gather(st, m, idx, as_float=as_float)
        _assert_gather(st, m, idx, as_float=as_float, names=["w", "q", "p"])


# ----------------------------------------------------------------------------- (h) random walk
def test_random_walk(ops):
    rng = np.random.RandomState(24)
    st, m = _make(ops, A_CAP, A_COLS)
    kinds = ["push", "stage", "push_device", "write_rows", "gather", "clear"]
    done = dict.fromkeys(kinds, 0)
    for step in range(300):
        kind = kinds[rng.choice(6, p=[0.22, 0.22, 0.22, 0.15, 0.15, 0.04])]
        done[kind] += 1
        if kind == "push":
            n = int(rng.randint(1, 3 * A_CAP))  # longer than the ring about half the time
            _append(st, m, _rows(rng, m, n), n, "push")
        elif kind in ("stage", "push_device"):
            n = int(rng.randint(1, A_CAP + 1))
            _append(st, m, _rows(rng, m, n), n, kind)
        elif kind == "write_rows":
            k = int(rng.randint(0, A_CAP + 1))
            slots = rng.permutation(A_CAP)[:k].astype(np.int64)
            if k and rng.rand() < 0.3:
                slots[rng.randint(k)] = [-1, A_CAP, 2**40][rng.randint(3)]
            rows = _rows(rng, m, k)
            st.write_rows(slots, rows)
            m.write_rows(slots, rows)
        elif kind == "gather":
            off = int(rng.choice([0, 0, 1000, -3]))
            idx = rng.randint(-2, A_CAP + 2, size=int(rng.randint(1, 80))) + off
            _assert_gather(st, m, idx, idx_offset=off, as_float={nm: bool(rng.randint(2)) for nm in m.names})
        else:
            st.clear()
            m.clear()
        _check(st, m, f"step {step}: {kind}")
    assert min(done.values()) >= 5, done
