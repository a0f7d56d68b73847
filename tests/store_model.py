"""Numpy model of the transition store (jh_store_*): the truth that tests/test_store_paths_gpu.py compares
ops.DeviceStore with, byte for byte.  No torch, no GPU.

The ring moves as core/buffer/replay_buffer.py:8-35 moves it (oracle.jorldy_oracle.ReplayOracle.store; pinned by
tests/test_store_model_cpu.py): row j of a push lands in slot (index + j) % capacity, so of a push longer than the
ring only the last `capacity` rows survive.  Slots that were never written hold a sentinel pattern, not zeros: a
row that never arrived and a neighbour that was overwritten both show in a whole-column comparison.
"""
import numpy as np

U8, F32, I64, F64, I32 = 0, 1, 2, 3, 4  # JH_U8 .. JH_I32 (include/jorldy_hip.h; asserted by the GPU test)
NP_OF = {U8: np.uint8, F32: np.float32, I64: np.int64, F64: np.float64, I32: np.int32}


def sentinel(capacity, elems, dtype, salt=0):
    """[capacity, elems] of `dtype` whose every BYTE depends on its position (period 127, a prime: no row size or
    16-byte piece divides it), so a piece that moved does not compare equal.  Bytes stay in 1..127, so every float
    is finite and normal (no NaN whose payload a cast could change)."""
    nbytes = capacity * elems * np.dtype(dtype).itemsize
    b = ((np.arange(nbytes, dtype=np.int64) * 7 + 13 + 31 * salt) % 127 + 1).astype(np.uint8)
    return b.view(dtype).reshape(capacity, elems).copy()


class StoreModel:
    def __init__(self, capacity, columns):
        """columns: list of (name, jh_dtype, elems[, shape]) as ops.DeviceStore takes them."""
        self.capacity = int(capacity)
        self.names = [c[0] for c in columns]
        self.dtype = {c[0]: np.dtype(NP_OF[c[1]]) for c in columns}
        self.elems = {c[0]: int(c[2]) for c in columns}
        self.cols = {nm: sentinel(self.capacity, self.elems[nm], self.dtype[nm], salt=k) for k, nm in enumerate(self.names)}
        self.index = 0
        self.counter = 0

    @property
    def size(self):
        return self.counter

    def _rows(self, cols, n=None):
        out = {}
        for nm in self.names:
            a = np.asarray(cols[nm])
            e = self.elems[nm]
            assert a.size % e == 0 and (n is not None or a.size == a.shape[0] * e), (nm, a.shape)
            a = a.reshape(-1, e) if n is None else a.reshape(-1)[: n * e].reshape(n, e)
            out[nm] = a.astype(self.dtype[nm])
        return out

    def push(self, cols, n=None):
        """Ring append of n rows (all of them when n is None), n > capacity included."""
        rows = self._rows(cols, n)
        n = len(rows[self.names[0]])
        slots = (self.index + np.arange(n)) % self.capacity
        keep = slice(max(0, n - self.capacity), n)  # earlier rows of a long push are overwritten by later ones
        for nm in self.names:
            self.cols[nm][slots[keep]] = rows[nm][keep]
        self.index = (self.index + n) % self.capacity
        self.counter = min(self.counter + n, self.capacity)
        return n

    def write_rows(self, slots, cols):
        """Row i lands in slot slots[i]; slots outside [0, capacity) are skipped; the ring position stays."""
        slots = np.asarray(slots, dtype=np.int64).reshape(-1)
        rows = self._rows(cols)
        ok = (slots >= 0) & (slots < self.capacity)
        assert np.unique(slots[ok]).size == ok.sum(), "which row wins a duplicated slot is not defined"
        for nm in self.names:
            assert len(rows[nm]) == slots.size
            self.cols[nm][slots[ok]] = rows[nm][ok]

    def clear(self):
        self.index = 0
        self.counter = 0

    def gather(self, idx, idx_offset=0, names=None, as_float=True):
        """dict name -> [B, elems]: rows clip(idx - idx_offset, 0, capacity - 1), float32 (numpy astype: round to
        nearest even) or the stored dtype; as_float may be a dict name -> bool (default True)."""
        names = self.names if names is None else names
        r = np.clip(np.asarray(idx, dtype=np.int64).reshape(-1) - int(idx_offset), 0, self.capacity - 1)
        out = {}
        for nm in names:
            f = as_float.get(nm, True) if isinstance(as_float, dict) else as_float
            v = self.cols[nm][r]
            with np.errstate(over="ignore"):  # a float64 beyond float32's range becomes inf, as on the GPU
                out[nm] = v.astype(np.float32) if f else v.copy()
        return out
