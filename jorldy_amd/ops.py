"""Torch-facing wrappers over the C ABI (device memory, streams: plumbing only).

Every function enqueues HIP kernels from libjorldy_hip.so on torch's current stream and
returns torch tensors that alias the outputs.  Nothing here computes on the CPU.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib as L

_DT = {torch.uint8: L.JH_U8, torch.float32: L.JH_F32, torch.int64: L.JH_I64, torch.float64: L.JH_F64, torch.int32: L.JH_I32, torch.bool: L.JH_U8}
_NP_DT = {np.dtype("uint8"): L.JH_U8, np.dtype("float32"): L.JH_F32, np.dtype("int64"): L.JH_I64, np.dtype("float64"): L.JH_F64, np.dtype("int32"): L.JH_I32, np.dtype("bool"): L.JH_U8}
_TORCH_OF = {L.JH_U8: torch.uint8, L.JH_F32: torch.float32, L.JH_I64: torch.int64, L.JH_F64: torch.float64, L.JH_I32: torch.int32}
_NP_OF = {L.JH_U8: np.uint8, L.JH_F32: np.float32, L.JH_I64: np.int64, L.JH_F64: np.float64, L.JH_I32: np.int32}


# ----------------------------------------------------------------------------- kernel timing
# bench.py measures the hand-written kernels live with HIP events recorded on the stream they are
# launched on (torch's current stream).  Off by default: zero overhead in the product path.
_PROF = {"on": False, "ev": {}, "lib": False}


class _timed:
    def __init__(self, name, nbytes, bound="hbm"):
        self.name, self.nbytes, self.bound = name, nbytes, bound

    def __enter__(self):
        if _PROF["on"]:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if _PROF["on"]:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _PROF["ev"].setdefault(self.name, []).append((self.e0, e1, self.nbytes, self.bound))


def profile_reset(enable):
    _PROF["on"] = bool(enable)
    _PROF["ev"] = {}


def profile_collect():
    """-> {kernel: (n_launches, total_ms, algorithmic_bytes_per_launch, bound)}"""
    torch.cuda.synchronize()
    out = {}
    for name, lst in _PROF["ev"].items():
        ms = sum(e0.elapsed_time(e1) for e0, e1, _, _ in lst)
        out[name] = (len(lst), ms, sum(x[2] for x in lst) / len(lst), lst[0][3])
    return out


def lib_profile(enable, repeat=1):
    """Bracket every kernel launched by libjorldy_hip with HIP events on its launch stream.  repeat > 1: the
    idempotent MFMA kernels run `repeat` times back to back inside one event pair (amortises the pair's ~4 us)."""
    _PROF["lib"] = bool(enable)
    L.check(L.load().jh_prof_enable(int(max(1, repeat)) if enable else 0))


def lib_profile_calibrate(n=64):
    """Record n empty event pairs (reported as "__event_pair_overhead")."""
    L.check(L.load().jh_prof_calibrate(int(n), L.stream_ptr()))


def lib_profile_report():
    """-> {kernel name: (launches, total_ms, total_flops)} (synchronises the device); flops only for the MFMA
    kernels that declare them, else 0."""
    buf = C.create_string_buffer(1 << 16)
    L.check(L.load().jh_prof_report(buf, len(buf)))
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, ms, work = line.split("\t")
        out[name] = (int(n), float(ms), float(work))
    return out


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda, "expected a float32 CUDA tensor"
    return t.contiguous()


def _dev(t):
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


# ============================================================================= store
class DeviceStore:
    """GPU-resident SoA ring of transitions (jh_store_*)."""

    def __init__(self, capacity, columns, device=None):
        """columns: list of (name, jh_dtype, elems, shape_without_batch)."""
        self.lib = L.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ctx = L.ctx(self.device.index)
        self.capacity = int(capacity)
        self.columns = list(columns)
        self.names = [c[0] for c in columns]
        descs = (L.ColDesc * len(columns))(*[L.ColDesc(int(c[1]), int(c[2])) for c in columns])
        self.h = C.c_void_p()
        L.check(self.lib.jh_store_create(self.ctx, self.capacity, len(columns), descs, C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_store_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def size(self):
        return int(self.lib.jh_store_size(self.h))

    @property
    def index(self):
        return int(self.lib.jh_store_index(self.h))

    def clear(self):
        self.lib.jh_store_clear(self.h)

    def push(self, cols):
        """cols: dict name -> numpy array [n, ...] (any float/int dtype; converted to the stored dtype)."""
        n = None
        arrs = []
        for name, dt, elems, _ in self.columns:
            src = np.asarray(cols[name]).reshape(len(cols[name]), -1)
            a = np.ascontiguousarray(src, dtype=_NP_OF[dt])
            if dt == L.JH_I64 and src.dtype.kind == "f" and not np.array_equal(a, src):
                raise ValueError(f"column {name} is stored as int64 (its first batch was integer-typed) but this batch holds fractional values")
            assert a.shape[1] == elems, f"column {name}: expected {elems} elems, got {a.shape[1]}"
            n = a.shape[0] if n is None else n
            assert a.shape[0] == n
            arrs.append(a)
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        L.check(self.lib.jh_store_push(self.h, n, ptrs, L.stream_ptr()))
        return n

    def write_rows(self, slots, cols):
        """Positional writes: row i of cols (dict name -> numpy [n, ...]) lands in slot slots[i]; the ring position
        is not touched (frame pool of the de-duplicated image replay)."""
        slots = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
        arrs = []
        for name, dt, elems, _ in self.columns:
            a = np.ascontiguousarray(np.asarray(cols[name]).reshape(-1, elems), dtype=_NP_OF[dt])  # (an empty call: zero rows)
            assert a.shape == (slots.size, elems)
            arrs.append(a)
        for o in range(0, slots.size, 32768):  # grid.y limit
            m = min(32768, slots.size - o)
            sub = (C.c_void_p * len(arrs))(*[a[o : o + m].ctypes.data for a in arrs])
            L.check(self.lib.jh_store_write_rows(self.h, m, slots[o : o + m].ctypes.data, sub, L.stream_ptr()))

    def push_device(self, cols, n):
        """cols: dict name -> CUDA tensor [n, ...] already in the stored dtype (device-to-device ring append)."""
        ts = []
        for name, dt, elems, _ in self.columns:
            t = cols[name].contiguous()
            assert t.is_cuda and t.dtype == _TORCH_OF[dt] and t.numel() >= n * elems
            ts.append(t)
        ptrs = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        L.check(self.lib.jh_store_push_device(self.h, int(n), ptrs, L.stream_ptr()))

    def stage(self, n):
        """Zero-copy push: returns dict name -> numpy view [n, elems] of PINNED memory; call commit() after filling."""
        ptrs = (C.c_void_p * len(self.columns))()
        L.check(self.lib.jh_store_stage_begin(self.h, n, ptrs))
        out = {}
        for (name, dt, elems, _), p in zip(self.columns, ptrs):
            buf = (C.c_char * (n * elems * np.dtype(_NP_OF[dt]).itemsize)).from_address(p)
            out[name] = np.frombuffer(buf, dtype=_NP_OF[dt]).reshape(n, elems)
        return out

    def commit(self):
        L.check(self.lib.jh_store_stage_commit(self.h, L.stream_ptr()))

    def column(self, name):
        """Zero-copy torch view of a whole device column [capacity, *shape] (the lib owns the memory)."""
        i = self.names.index(name)
        _, dt, elems, shape = self.columns[i]
        p = self.lib.jh_store_col_ptr(self.h, i)
        return _wrap_device(p, (self.capacity,) + tuple(shape), _TORCH_OF[dt], self.device, owner=self)

    def gather(self, idx, names=None, as_float=True, idx_offset=0, out=None):
        """idx: int64 CUDA tensor [B] -> dict name -> tensor [B, *shape]; float32 (as_tensor semantics)
        unless as_float=False (stored dtype, e.g. uint8 frames)."""
        names = self.names if names is None else names
        B = int(idx.numel())
        sel, outs, odt = [], [], []
        for nm in names:
            i = self.names.index(nm)
            _, dt, elems, shape = self.columns[i]
            keep = (not as_float) if not isinstance(as_float, dict) else (not as_float.get(nm, True))
            tdt = _TORCH_OF[dt] if keep else torch.float32
            if out is not None:  # static output buffers (graph capture / no allocator traffic)
                o_t = out[nm]
                assert o_t.dtype == tdt and o_t.is_contiguous() and o_t.numel() == B * elems
                outs.append(o_t)
            else:
                outs.append(torch.empty((B,) + tuple(shape), dtype=tdt, device=self.device))
            sel.append(i)
            odt.append(_DT[tdt])
        if B == 0:  # nothing to launch (an empty idx has no device pointer to pass)
            return dict(zip(names, outs))
        selc = (C.c_int32 * len(sel))(*sel)
        odtc = (C.c_int32 * len(sel))(*odt)
        ptrs = (C.c_void_p * len(sel))(*[o.data_ptr() for o in outs])
        assert idx.dtype == torch.int64 and idx.is_cuda
        nbytes = sum(B * self.columns[i][2] * np.dtype(_NP_OF[self.columns[i][1]]).itemsize + o.numel() * o.element_size() for i, o in zip(sel, outs)) + 8 * B
        with _timed("jh_gather_kernel", nbytes):
            L.check(self.lib.jh_store_gather(self.h, B, L.ptr(idx.contiguous()), int(idx_offset), len(sel), selc, ptrs, odtc, L.stream_ptr()))
        return dict(zip(names, outs))


class _Owner:
    pass


def _wrap_device(ptr_value, shape, dtype, device, owner=None):
    """torch tensor aliasing raw device memory owned by the library (via __cuda_array_interface__)."""
    typestr = {torch.uint8: "|u1", torch.float32: "<f4", torch.int64: "<i8", torch.float64: "<f8", torch.int32: "<i4"}[dtype]
    holder = _Owner()
    holder.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr_value), False), "version": 2}
    holder._owner = owner
    with torch.cuda.device(device):
        return torch.as_tensor(holder, device=device)


# ============================================================================= PER sum tree
class ActorFeed:
    """jh_feed_*: per-tick frame-stack de-duplication + Ape-X n-step assembly with actor-side priorities for N lockstep
    actors, entirely in HBM (core/env/atari.py:145-149 + core/agent/ape_x.py:174-199; csrc/jh_feed.hip)."""

    def __init__(self, n_actors, channels, plane_bytes, n_step, gamma, planes_per_actor, window_ticks, device=None):
        self.lib = L.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.N, self.C, self.n, self.plane = int(n_actors), int(channels), int(n_step), int(plane_bytes)
        self.h = C.c_void_p()
        L.check(self.lib.jh_feed_create(L.ctx(self.device.index), self.N, self.C, self.plane, self.n, float(gamma), int(planes_per_actor),
                                        int(window_ticks), C.byref(self.h)))
        self._rew = np.empty(self.N, np.float32)
        self._done = np.empty(self.N, np.float32)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_feed_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def tick(self, obs, prev_obs, pool, action, q, reward, done, out, prio_eps=0.0):
        """obs / prev_obs uint8 [N, C, ...] (device; prev_obs None on the first tick), pool = the plane pool column
        (device), action int64 [N] / q float32 [N] (device), reward / done: host arrays [N].  out: dict of preallocated
        device tensors state int64 [N, C], next_state int64 [N, C], action int64 [N], reward float32 [N, n],
        done uint8 [N, n], priority float64 [N].  Returns the number of transitions emitted (0 or N), enqueued on the
        current stream."""
        for t in (obs, pool, action, q):
            assert t.is_cuda and t.is_contiguous()
        assert obs.dtype == torch.uint8 and action.dtype == torch.int64 and q.dtype == torch.float32
        assert out["state"].dtype == torch.int64 and out["reward"].dtype == torch.float32 and out["done"].dtype == torch.uint8 and out["priority"].dtype == torch.float64
        np.copyto(self._rew, np.asarray(reward, dtype=np.float32).reshape(-1))
        np.copyto(self._done, np.asarray(done, dtype=np.float32).reshape(-1))
        emitted = C.c_int32(0)
        L.check(self.lib.jh_feed_tick(self.h, L.ptr(obs), L.ptr(prev_obs), L.ptr(pool), L.ptr(action), L.ptr(q), L.ptr(self._rew), L.ptr(self._done),
                                      float(prio_eps), L.ptr(out["state"]), L.ptr(out["next_state"]), L.ptr(out["action"]), L.ptr(out["reward"]),
                                      L.ptr(out["done"]), L.ptr(out["priority"]), C.byref(emitted), L.stream_ptr()))
        return int(emitted.value)

    def save_state(self):
        """The feed's own state (device block + tick) as bytes (jh_feed_save; synchronises the current stream)."""
        n = int(self.lib.jh_feed_state_bytes(self.h))
        buf = np.empty(n, np.uint8)
        L.check(self.lib.jh_feed_save(self.h, L.ptr(buf), n, L.stream_ptr()))
        return buf

    def load_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        L.check(self.lib.jh_feed_load(self.h, L.ptr(buf), int(buf.size), L.stream_ptr()))

    def push_stacks(self, obs, prev_obs, pool):
        """First half of a tick, stack mode (see tick)."""
        L.check(self.lib.jh_feed_push_stacks(self.h, L.ptr(obs), L.ptr(prev_obs), L.ptr(pool), L.stream_ptr()))

    def push_frames(self, frames, reset, pool, stack_out):
        """First half of a tick, frame mode: frames uint8 [N, ...] (device) = the newest plane of every actor, reset: host
        flags [N]; stack_out uint8 [N, C, ...] (device) <- the rebuilt stacks for the acting forward."""
        assert frames.is_cuda and frames.is_contiguous() and frames.dtype == torch.uint8 and stack_out.is_cuda and stack_out.is_contiguous()
        r = np.ascontiguousarray(np.asarray(reset).reshape(-1), dtype=np.uint8)
        assert r.size == self.N
        L.check(self.lib.jh_feed_push_frames(self.h, L.ptr(frames), L.ptr(r), L.ptr(pool), L.ptr(stack_out), L.stream_ptr()))

    def emit(self, action, q, reward, done, out, prio_eps=0.0):
        """Second half of a tick (see tick for the arguments); returns the number of transitions emitted (0 or N)."""
        assert action.is_cuda and action.dtype == torch.int64 and q.is_cuda and q.dtype == torch.float32
        np.copyto(self._rew, np.asarray(reward, dtype=np.float32).reshape(-1))
        np.copyto(self._done, np.asarray(done, dtype=np.float32).reshape(-1))
        emitted = C.c_int32(0)
        L.check(self.lib.jh_feed_emit(self.h, L.ptr(action), L.ptr(q), L.ptr(self._rew), L.ptr(self._done), float(prio_eps), L.ptr(out["state"]),
                                      L.ptr(out["next_state"]), L.ptr(out["action"]), L.ptr(out["reward"]), L.ptr(out["done"]), L.ptr(out["priority"]),
                                      C.byref(emitted), L.stream_ptr()))
        return int(emitted.value)

    def state(self):
        """(flags, planes written so far); blocking."""
        fl, pw = C.c_int32(0), C.c_int64(0)
        L.check(self.lib.jh_feed_state(self.h, C.byref(fl), C.byref(pw), L.stream_ptr()))
        return int(fl.value), int(pw.value)


class SumTree:
    """Device float64 sum tree (jh_per_*), bit-identical to per_buffer.py's numpy tree."""

    def __init__(self, capacity, uniform_sample_prob=1e-3, device=None):
        self.lib = L.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.ctx = L.ctx(self.device.index)
        self.capacity = int(capacity)
        self.usp = float(uniform_sample_prob)
        self.h = C.c_void_p()
        L.check(self.lib.jh_per_create(self.ctx, self.capacity, self.usp, C.byref(self.h)))
        # {sampled_p, mean_p, root, max_w} of the last sample: device-mapped pinned memory, so that a learner can read
        # them without a copy + stream sync once it knows the sampling kernel has finished (`stats_np`)
        self._stats = PinnedBuffer((4,), np.float64, self.device)
        self.stats_np = self._stats.np

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_per_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def tree_size(self):
        return 2 * self.capacity - 1

    def push(self, n, priorities=None):
        p = None if priorities is None else np.ascontiguousarray(priorities, dtype=np.float64).reshape(-1)
        if p is not None:
            assert p.size == n
        L.check(self.lib.jh_per_push(self.h, int(n), L.ptr(p), L.stream_ptr()))

    def push_device(self, n, priorities):
        """push() with float64 priorities that are already on the device (ActorFeed's actor-side priorities)."""
        assert priorities.is_cuda and priorities.dtype == torch.float64 and priorities.is_contiguous() and priorities.numel() >= n
        L.check(self.lib.jh_per_push_device(self.h, int(n), L.ptr(priorities), L.stream_ptr()))

    def update(self, idx, prio):
        assert idx.dtype == torch.int64 and idx.is_cuda and prio.is_cuda
        dt = L.JH_F32 if prio.dtype == torch.float32 else L.JH_F64
        assert prio.dtype in (torch.float32, torch.float64)
        L.check(self.lib.jh_per_update(self.h, int(idx.numel()), L.ptr(idx.contiguous()), L.ptr(prio.contiguous()), dt, L.stream_ptr()))

    def sample(self, beta, uniform_slot, u, want_w64=True, out_idx=None, out_w32=None):
        """uniform_slot int64[n_uni] (numpy), u float64[B-n_uni] (numpy).  Returns (idx i64[B], w64|None, w32, stats f64[4]) on device.
        out_idx / out_w32: preallocated outputs (static buffers of a captured graph)."""
        uniform_slot = np.ascontiguousarray(uniform_slot, dtype=np.int64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        B = uniform_slot.size + u.size
        idx = torch.empty(B, dtype=torch.int64, device=self.device) if out_idx is None else out_idx
        w64 = torch.empty(B, dtype=torch.float64, device=self.device) if want_w64 else None
        w32 = torch.empty(B, dtype=torch.float32, device=self.device) if out_w32 is None else out_w32
        assert idx.numel() == B and w32.numel() == B
        L.check(self.lib.jh_per_sample(self.h, B, float(beta), int(uniform_slot.size), L.ptr(uniform_slot), L.ptr(u), L.ptr(idx), L.ptr(w64), L.ptr(w32), L.ptr(self._stats.dev), L.stream_ptr()))
        return idx, w64, w32, self._stats.dev

    def shard_stats(self, B, out3):
        """out3 (float64 [3], device) <- {root, count, min priority of the last sample of B}."""
        L.check(self.lib.jh_per_shard_stats(self.h, int(B), L.ptr(out3), L.stream_ptr()))

    def weights_sharded(self, B, beta, all3, w32):
        """IS weights of the last sample against the logical buffer described by the gathered triples all3 [G, 3]."""
        L.check(self.lib.jh_per_weights_sharded(self.h, int(B), float(beta), L.ptr(all3), int(all3.numel() // 3), None, L.ptr(w32), L.stream_ptr()))

    def view(self):
        """Zero-copy float64 [2N-1] torch view of the device tree (the library owns the memory)."""
        return _wrap_device(self.lib.jh_per_tree_ptr(self.h), (self.tree_size,), torch.float64, self.device, owner=self)

    def state(self):
        mp, root, ti, cnt = C.c_double(), C.c_double(), C.c_int64(), C.c_int64()
        L.check(self.lib.jh_per_state(self.h, C.byref(mp), C.byref(root), C.byref(ti), C.byref(cnt), L.stream_ptr()))
        return dict(max_priority=mp.value, root=root.value, tree_index=ti.value, counter=cnt.value)

    def dump(self):
        out = np.empty(self.tree_size, dtype=np.float64)
        L.check(self.lib.jh_per_dump(self.h, L.ptr(out), L.stream_ptr()))
        return out

    def load(self, tree, max_priority, tree_index, counter):
        t = np.ascontiguousarray(tree, dtype=np.float64)
        assert t.size == self.tree_size
        L.check(self.lib.jh_per_load(self.h, L.ptr(t), float(max_priority), int(tree_index), int(counter)))


# ============================================================================= PPO math
def gae(reward, done, value, next_value, n_step, gamma, lam, standardize=True, out=None):
    """ppo.py:95-110.  Inputs float32 CUDA [M,1] (or [M]), M = W*n_step, worker-major.
    Returns (adv [M,1], ret [M,1]); `out` = preallocated (adv, ret)."""
    lib = L.load()
    r, d, v, vn = (_f32(x).reshape(-1) for x in (reward, done, value, next_value))
    M = r.numel()
    assert M % n_step == 0
    if out is None:
        adv = torch.empty(M, dtype=torch.float32, device=r.device)
        ret = torch.empty(M, dtype=torch.float32, device=r.device)
    else:
        adv, ret = (_f32(t).reshape(-1) for t in out)
    with _timed("jh_gae_kernel", 24 * M):  # 4 reads + 2 writes of fp32 per transition
      L.check(lib.jh_gae(L.ctx(_dev(r)), M // n_step, int(n_step), float(gamma), float(lam), L.ptr(r), L.ptr(d), L.ptr(v), L.ptr(vn), L.ptr(adv), L.ptr(ret), int(bool(standardize)), L.stream_ptr()))
    return adv.view(-1, 1), ret.view(-1, 1)


def mean_into(x, out):
    """out[0] = mean(x) (ppo.py:112), one deterministic workgroup."""
    x = _f32(x).reshape(-1)
    L.check(L.load().jh_mean_f32(L.ctx(_dev(x)), int(x.numel()), L.ptr(x), L.ptr(out), L.stream_ptr()))
    return out


class MinibatchRows:
    """jh_ppo_minibatch_rows: the `x[idx]` gathers of every epoch of ppo.py:118-125 done once per learn().
    srcs / dsts: lists of float32 CUDA tensors [M, e_c] / [n, e_c] (static addresses: capturable)."""

    def __init__(self, srcs, dsts):
        self.lib = L.load()
        assert len(srcs) == len(dsts) <= 8
        self.srcs, self.dsts = [_f32(t) for t in srcs], list(dsts)
        n = len(srcs)
        self.n = int(dsts[0].shape[0])
        el = [int(t.numel() // t.shape[0]) for t in self.srcs]
        assert all(int(d.numel()) == self.n * e and d.is_contiguous() for d, e in zip(self.dsts, el))
        self._elems = (C.c_int32 * n)(*el)
        self._src = (C.c_void_p * n)(*[t.data_ptr() for t in self.srcs])
        self._dst = (C.c_void_p * n)(*[t.data_ptr() for t in self.dsts])
        self.ctx = L.ctx(_dev(self.srcs[0]))

    def __call__(self, idx):
        assert idx.dtype == torch.int64 and int(idx.numel()) == self.n
        L.check(self.lib.jh_ppo_minibatch_rows(self.ctx, self.n, L.ptr(idx), len(self.srcs), self._elems, self._src, self._dst, L.stream_ptr()))
        return self.dsts


def logp_discrete(logits, action, out=None):
    lib = L.load()
    z = _f32(logits)
    M, A = z.shape
    a = _f32(action).reshape(-1)
    out = torch.empty(M, dtype=torch.float32, device=z.device) if out is None else _f32(out).reshape(-1)
    L.check(lib.jh_logp_discrete(L.ctx(_dev(z)), M, A, L.ptr(z), L.ptr(a), L.ptr(out), L.stream_ptr()))
    return out.view(-1, 1)


def logp_continuous(mu_raw, log_std_raw, action, out=None):
    lib = L.load()
    mu, ls, a = _f32(mu_raw), _f32(log_std_raw), _f32(action)
    M, A = mu.shape
    out = torch.empty(M, A, dtype=torch.float32, device=mu.device) if out is None else _f32(out)
    L.check(lib.jh_logp_continuous(L.ctx(_dev(mu)), M, A, L.ptr(mu), L.ptr(ls), L.ptr(a), L.ptr(out), L.stream_ptr()))
    return out


def ppo_loss_discrete(logits, value_pred, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, stats=None):
    """Returns (grad_logits [B,A], grad_value [B,1], stats f32[8])."""
    lib = L.load()
    z, v = _f32(logits), _f32(value_pred).reshape(-1)
    B, A = z.shape
    g_z = torch.empty_like(z)
    g_v = torch.empty(B, dtype=torch.float32, device=z.device)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=z.device)
    with _timed("jh_ppo_fused_kernel" if B <= 1024 else "jh_ppo_fwd+bwd", 4 * B * (2 * A + 7) + 8 * B):  # (A+6) reads + (A+1) writes + idx
      L.check(lib.jh_ppo_loss_discrete(L.ctx(_dev(z)), B, A, L.ptr(z), L.ptr(v), L.ptr(idx), L.ptr(_f32(action).reshape(-1)), L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)), L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(logp_old).reshape(-1)), float(eps_clip), float(vf_coef), float(ent_coef), L.ptr(g_z), L.ptr(g_v), L.ptr(stats), L.stream_ptr()))
    return g_z, g_v.view(-1, 1), stats


def ppo_loss_continuous(mu_raw, log_std_raw, value_pred, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, stats=None):
    lib = L.load()
    mu, ls, v = _f32(mu_raw), _f32(log_std_raw), _f32(value_pred).reshape(-1)
    B, A = mu.shape
    g_mu, g_ls = torch.empty_like(mu), torch.empty_like(ls)
    g_v = torch.empty(B, dtype=torch.float32, device=mu.device)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=mu.device)
    L.check(lib.jh_ppo_loss_continuous(L.ctx(_dev(mu)), B, A, L.ptr(mu), L.ptr(ls), L.ptr(v), L.ptr(idx), L.ptr(_f32(action)), L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)), L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(logp_old)), float(eps_clip), float(vf_coef), float(ent_coef), L.ptr(g_mu), L.ptr(g_ls), L.ptr(g_v), L.ptr(stats), L.stream_ptr()))
    return g_mu, g_ls, g_v.view(-1, 1), stats


def ppo_loss_dp(head0, head1, value_pred, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, stats, reduce_mean, work):
    """ppo_loss_discrete (head1 None) / ppo_loss_continuous for data-parallel learners with the global critic branch (jh_ppo_loss_deferred ->
    reduce_mean(critic sums) -> jh_ppo_critic_select_rows).  work: fp32 device tensor of >= B + 16 elements (second branch's value gradients,
    the two sums, the local statistics row).  Returns the head gradients like the plain functions."""
    lib = L.load()
    cont = head1 is not None
    h0, v = _f32(head0), _f32(value_pred).reshape(-1)
    h1 = _f32(head1) if cont else None
    B, A = h0.shape
    g0 = torch.empty_like(h0)
    g1 = torch.empty_like(h1) if cont else None
    g_v = torch.empty(B, dtype=torch.float32, device=h0.device)
    dv2, sums, local = work[:B], work[B : B + 2], work[B + 8 : B + 16]
    ctx = L.ctx(_dev(h0))
    L.check(lib.jh_ppo_loss_deferred(ctx, int(cont), B, A, L.ptr(h0), L.ptr(h1), L.ptr(v), L.ptr(idx), L.ptr(_f32(action) if cont else _f32(action).reshape(-1)),
                                     L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)), L.ptr(_f32(value_old).reshape(-1)),
                                     L.ptr(_f32(logp_old) if cont else _f32(logp_old).reshape(-1)), float(eps_clip), float(vf_coef), float(ent_coef),
                                     L.ptr(g0), L.ptr(g1), L.ptr(g_v), L.ptr(dv2), L.ptr(sums), L.ptr(local), L.stream_ptr()))
    reduce_mean(sums)
    L.check(lib.jh_ppo_critic_select_rows(ctx, B, L.ptr(sums), float(vf_coef), float(ent_coef), L.ptr(g_v), L.ptr(dv2), L.ptr(local), L.ptr(stats), L.stream_ptr()))
    return (g0, g1, g_v.view(-1, 1)) if cont else (g0, g_v.view(-1, 1))


def ppo_loss_packed(heads, A, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, grad_out, stats, continuous=False, reduce_mean=None, work=None):
    """The PPO losses (ppo.py:122-165) on a network whose last layer stacks the heads (jh_ppo_loss_packed): heads float32 [B, ld] = (head0 [A] | head1 [A]
    (continuous) | value | padding), grad_out the same shape -- d(loss)/d(heads), padding columns untouched (keep them zero).  idx None: the per-row
    inputs are already the minibatch's rows.  reduce_mean + work (>= B + 16 floats): data-parallel learners, the critic branch of the GLOBAL minibatch
    (ppo_loss_dp's scheme)."""
    lib = L.load()
    assert heads.dtype == torch.float32 and heads.is_contiguous() and grad_out.is_contiguous() and grad_out.shape == heads.shape
    B, ld = int(heads.shape[0]), int(heads.shape[1])
    ctx = L.ctx(_dev(heads))
    act = _f32(action) if continuous else _f32(action).reshape(-1)
    lpo = _f32(logp_old) if continuous else _f32(logp_old).reshape(-1)
    dv2 = sums = local = None
    if reduce_mean is not None:
        dv2, sums, local = work[:B], work[B : B + 2], work[B + 8 : B + 16]
    L.check(lib.jh_ppo_loss_packed(ctx, int(bool(continuous)), B, int(A), L.ptr(heads), ld, L.ptr(idx), L.ptr(act), L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)),
                                   L.ptr(_f32(value_old).reshape(-1)), L.ptr(lpo), float(eps_clip), float(vf_coef), float(ent_coef), L.ptr(grad_out), L.ptr(dv2), L.ptr(sums),
                                   L.ptr(local if reduce_mean is not None else stats), L.stream_ptr()))
    if reduce_mean is not None:
        reduce_mean(sums)
        nv = (2 * A if continuous else A)
        gv = grad_out.view(-1)[nv:]  # the value column, row stride ld
        L.check(lib.jh_ppo_critic_select_strided(ctx, B, L.ptr(sums), float(vf_coef), float(ent_coef), L.ptr(gv), ld, L.ptr(dv2), L.ptr(local), L.ptr(stats), L.stream_ptr()))
    return grad_out


def heads_unpack(packed, A, h0, h1, value):
    """packed [rows, ld] -> h0 [rows, A], h1 [rows, A] (or None), value [rows]: the layout jh_logp_* / jh_gae read."""
    assert packed.is_contiguous() and h0.is_contiguous() and value.is_contiguous() and (h1 is None or h1.is_contiguous())
    L.check(L.load().jh_heads_unpack(L.ctx(_dev(packed)), int(packed.shape[0]), int(A), L.ptr(packed), int(packed.shape[1]), L.ptr(h0), L.ptr(h1), L.ptr(value), L.stream_ptr()))


def rnd_adv_mix(adv_e, adv_i, ret, ret_i, n_step, extrinsic_coeff, intrinsic_coeff, standardize, out, means):
    """rnd_ppo.py:153-166 behind two gae(..., standardize=False) calls: out [M] = ext * adv_e + int * adv_i, standardised per row of n_step
    entries (unbiased std, + 1e-7) when asked; means [2] = mean(ret), mean(ret_i)."""
    a_e, a_i, r_e, r_i, o = (_f32(t).reshape(-1) for t in (adv_e, adv_i, ret, ret_i, out))
    M = int(a_e.numel())
    assert M % int(n_step) == 0 and all(int(t.numel()) == M for t in (a_i, r_e, r_i, o)) and means.numel() >= 2 and means.is_contiguous()
    L.check(L.load().jh_rnd_adv_mix(L.ctx(_dev(a_e)), M // int(n_step), int(n_step), float(extrinsic_coeff), float(intrinsic_coeff), int(bool(standardize)), L.ptr(a_e),
                                    L.ptr(a_i), L.ptr(r_e), L.ptr(r_i), L.ptr(o), L.ptr(means), L.stream_ptr()))
    return out


def rnd_ppo_loss_packed(heads, A, idx, action, adv, ret, ret_i, value_old, vi_old, logp_old, eps_clip, vf_coef, ent_coef, grad_out, stats, continuous=False):
    """RND-PPO's losses (rnd_ppo.py:201-249) on heads float32 [B, ld] = (head0 [A] | head1 [A] (continuous) | v | v_i | padding); grad_out the same
    shape, padding columns untouched.  idx None: the per-row inputs are already the minibatch's rows.  stats [8] = 0, actor, critic_e, critic_i,
    entropy, max ratio, min prob, 0."""
    assert heads.dtype == torch.float32 and heads.is_contiguous() and grad_out.is_contiguous() and grad_out.shape == heads.shape
    assert stats is None or (stats.numel() >= 8 and stats.is_contiguous())
    B, ld = int(heads.shape[0]), int(heads.shape[1])
    act = _f32(action) if continuous else _f32(action).reshape(-1)
    lpo = _f32(logp_old) if continuous else _f32(logp_old).reshape(-1)
    per_row = [_f32(t).reshape(-1) for t in (adv, ret, ret_i, value_old, vi_old)]
    rows = int(per_row[0].numel())
    assert all(int(t.numel()) == rows for t in per_row) and int(act.numel()) == rows * (A if continuous else 1) and int(lpo.numel()) == int(act.numel())
    assert idx is not None or rows >= B
    L.check(L.load().jh_rnd_ppo_loss_packed(L.ctx(_dev(heads)), int(bool(continuous)), B, int(A), L.ptr(heads), ld, L.ptr(idx), L.ptr(act), *(L.ptr(t) for t in per_row[:3]),
                                            L.ptr(per_row[3]), L.ptr(per_row[4]), L.ptr(lpo), float(eps_clip), float(vf_coef), float(ent_coef), L.ptr(grad_out),
                                            L.ptr(stats), L.stream_ptr()))
    return grad_out


def policy_act_discrete(heads, A, seed, counter, training, out):
    """ppo.py:63-69 on device-resident heads [W, ld]: out int64 [W] (device / device-mapped) <- sampled (training) or greedy actions."""
    assert heads.is_contiguous() and out.dtype == torch.int64
    L.check(L.load().jh_policy_act_discrete(L.ctx(_dev(heads)), int(heads.shape[0]), int(A), L.ptr(heads), int(heads.shape[1]), int(seed) & (2**64 - 1), int(counter) & (2**64 - 1),
                                            int(bool(training)), L.ptr(out), L.stream_ptr()))
    return out


# ============================================================================= V-MPO
VMPO_BLOCK_FLOATS = 24
_VMPO_NAMES = ("eta", "alpha_mu", "alpha_sigma")


def vmpo_block(eta=1.0, alpha_mu=1.0, alpha_sigma=1.0, min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.02, eps_alpha_mu=0.1, eps_alpha_sigma=0.1,
               m=(0.0, 0.0, 0.0), v=(0.0, 0.0, 0.0), has_state=(False, False, False), device="cuda"):
    """The Lagrange multipliers' device block of the jh_vmpo_* kernels (include/jorldy_hip.h): values (already raised to their floors, as the
    constructor's reset_lgr_muls does, vmpo.py:85), Adam's moments, floors, thresholds, the has-state flags.  -> float32 [24] on `device`."""
    h = np.zeros(VMPO_BLOCK_FLOATS, np.float32)
    h[9:12] = [min_eta, min_alpha_mu, min_alpha_sigma]
    h[0:3] = np.maximum(np.asarray([eta, alpha_mu, alpha_sigma], np.float32), h[9:12])
    h[3:6], h[6:9] = m, v
    h[12:15] = [eps_eta, eps_alpha_mu, eps_alpha_sigma]
    h[15:18] = [1.0 if f else 0.0 for f in has_state]
    return torch.from_numpy(h).to(device)


def vmpo_block_read(block):
    """-> {"eta": {"value", "m", "v", "floor", "eps", "has_state", "grad"}, "alpha_mu": ..., "alpha_sigma": ...} as Python numbers."""
    h = block.detach().cpu().numpy()
    return {k: {"value": float(h[j]), "m": float(h[3 + j]), "v": float(h[6 + j]), "floor": float(h[9 + j]), "eps": float(h[12 + j]),
                "has_state": bool(h[15 + j]), "grad": float(h[18 + j])} for j, k in enumerate(_VMPO_NAMES)}


def vmpo_block_moments(block):
    """-> (m, v) of the three multipliers as an optimizer holds them: 0-dim float32 tensors on the block's device, None where the has-state
    flag is off (alpha_sigma of a discrete policy never takes a step).  Synchronises."""
    h = block.detach().cpu()
    return tuple([h[o + j].clone().to(block.device) if h[15 + j] else None for j in range(3)] for o in (3, 6))


def _vmpo_block_write(block, h):
    torch.cuda.current_stream().synchronize()
    block.copy_(torch.from_numpy(np.asarray(h, np.float32)))


def vmpo_block_set_moments(block, m, v):
    """The inverse, in place: m / v [3] of one-element tensors, None = no optimizer state (moments 0, flag off).  The values stay."""
    h = block.detach().cpu().numpy().copy()
    for j in range(3):
        h[3 + j], h[6 + j], h[15 + j] = (0.0, 0.0, 0.0) if v[j] is None else (float(m[j]), float(v[j]), 1.0)
    _vmpo_block_write(block, h)


def vmpo_block_hex(block):
    """The whole block as the list of strings the resume manifest stores: exact, and a NaN survives JSON."""
    return [float(x).hex() for x in block.detach().cpu().numpy().astype(np.float64)]


def vmpo_block_from_hex(block, hexes):
    _vmpo_block_write(block, [float.fromhex(x) for x in hexes])


def vmpo_hyper(lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0, device="cuda"):
    """A hand-made optimizer block in the layout of jh_pponet_hyper_ptr (16 floats: lr, betas, eps, step, ..., the betas as doubles at
    [10:14]) for calling the V-MPO loss kernels without a network.  `step` = Adam steps taken BEFORE the coming one."""
    h = np.zeros(16, np.float32)
    h[:5] = [lr, beta1, beta2, eps, step]
    h[7:9] = [1.0 - beta1, 1.0 - beta2]
    h[10:14] = np.asarray([beta1, beta2], np.float64).view(np.float32)
    return torch.from_numpy(h).to(device)


def _mult_args(block, hyper, device):
    """The multiplier block of a loss call of the MPO family, checked, and `hyper` (a vmpo_hyper tensor or a net's hyper_ptr()) as a c_void_p."""
    assert block.dtype == torch.float32 and block.numel() == VMPO_BLOCK_FLOATS and block.is_contiguous()
    if not torch.is_tensor(hyper):
        return C.c_void_p(int(hyper))
    assert hyper.dtype == torch.float32 and hyper.numel() >= 16 and hyper.is_contiguous() and hyper.device == device
    return C.c_void_p(hyper.data_ptr())


def _stats_arg(stats, n, device):
    """stats: made (zeros) where None, checked to hold n floats where given."""
    if stats is None:
        return torch.zeros(n, dtype=torch.float32, device=device)
    assert stats.dtype == torch.float32 and stats.numel() >= n and stats.is_contiguous()
    return stats


def _out_arg(out, like, at_least=False):
    """out: a tensor a loss call writes a gradient into, made like `like` where None, checked to hold its floats (exactly, or at least) where given."""
    if out is None:
        return torch.empty_like(like)
    assert out.is_contiguous() and out.dtype == torch.float32 and (out.numel() >= like.numel() if at_least else out.numel() == like.numel())
    return out


def _vmpo_common(head, value_pred, idx, block, hyper, stats, mask):
    B, A = head.shape
    assert idx is None or (idx.dtype == torch.int64 and idx.numel() == B and idx.is_contiguous())
    hyper_ptr = _mult_args(block, hyper, head.device)
    g_v = torch.empty(B, dtype=torch.float32, device=head.device)
    assert mask is None or (mask.dtype == torch.float32 and mask.numel() >= B and mask.is_contiguous())
    return B, A, hyper_ptr, g_v, _stats_arg(stats, 8, head.device)


def vmpo_loss_discrete(logits, value_pred, idx, action, adv, value_old, logits_old, block, hyper, stats=None, mask=None):
    """jh_vmpo_loss_discrete: the minibatch's logits [B, A] and value_pred [B], idx int64 [B] into the rollout-sized action / adv / value_old /
    logits_old.  `block` (vmpo_block) is advanced in place; hyper = a net's hyper_ptr() or a vmpo_hyper tensor.
    -> (grad_logits [B, A], grad_value [B, 1], stats f32[8] = actor, critic, eta_loss, alpha_loss, eta', alpha_mu', alpha_sigma', mark)."""
    z, v = _f32(logits), _f32(value_pred).reshape(-1)
    B, A, hyper_ptr, g_v, stats = _vmpo_common(z, v, idx, block, hyper, stats, mask)
    g_z = torch.empty_like(z)
    L.check(L.load().jh_vmpo_loss_discrete(L.ctx(_dev(z)), B, A, L.ptr(z), L.ptr(v), L.ptr(idx), L.ptr(_f32(action).reshape(-1)), L.ptr(_f32(adv).reshape(-1)),
                                           L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(logits_old)), L.ptr(block), hyper_ptr, L.ptr(g_z), L.ptr(g_v), L.ptr(stats),
                                           L.ptr(mask), L.stream_ptr()))
    return g_z, g_v.view(-1, 1), stats


def vmpo_loss_continuous(mu_raw, log_std_raw, value_pred, idx, action, adv, value_old, mu_raw_old, log_std_raw_old, block, hyper, stats=None, mask=None):
    """jh_vmpo_loss_continuous, as vmpo_loss_discrete with the raw Gaussian heads -> (grad_mu_raw, grad_log_std_raw, grad_value [B, 1], stats)."""
    mu, ls, v = _f32(mu_raw), _f32(log_std_raw), _f32(value_pred).reshape(-1)
    B, A, hyper_ptr, g_v, stats = _vmpo_common(mu, v, idx, block, hyper, stats, mask)
    assert tuple(ls.shape) == (B, A)
    g_mu, g_ls = torch.empty_like(mu), torch.empty_like(ls)
    L.check(L.load().jh_vmpo_loss_continuous(L.ctx(_dev(mu)), B, A, L.ptr(mu), L.ptr(ls), L.ptr(v), L.ptr(idx), L.ptr(_f32(action)), L.ptr(_f32(adv).reshape(-1)),
                                             L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(mu_raw_old)), L.ptr(_f32(log_std_raw_old)), L.ptr(block), hyper_ptr,
                                             L.ptr(g_mu), L.ptr(g_ls), L.ptr(g_v), L.ptr(stats), L.ptr(mask), L.stream_ptr()))
    return g_mu, g_ls, g_v.view(-1, 1), stats


# ============================================================================= MPO
MPO_STATS = ("actor_loss", "critic_loss", "eta_loss", "alpha_loss", "eta", "alpha_mu", "alpha_sigma", "min_Q", "max_Q", "min_At", "max_At")


def mpo_loss_discrete(la, la_next, la_old, q, qt, qt_next, action, reward, done, prob_b, T, block, hyper, gamma, retrace=True, stats=None, out=None):
    """jh_mpo_loss_discrete: actor logits online(s), online(s'), target(s) and critic online(s), target(s), target(s'), each [R, A] with
    R = batch * T rows (row b * T + t), the replayed columns [R]; `block` (vmpo_block) is advanced in place with the ACTOR's optimizer block
    `hyper` (RainbowNet.hyper_ptr() or a vmpo_hyper tensor).  out = (grad_la, grad_q) to write into.
    -> (grad_la [R, A], grad_q [R, A], stats f32[11] in the order of MPO_STATS)."""
    t = [_f32(v) for v in (la, la_next, la_old, q, qt, qt_next)]
    R, A = t[0].shape
    assert all(tuple(v.shape) == (R, A) for v in t)
    cols = [_f32(v).reshape(-1) for v in (action, reward, done, prob_b)]
    assert all(v.numel() == R for v in cols)
    hyper_ptr = _mult_args(block, hyper, t[0].device)
    g_la, g_q = out if out is not None else (None, None)
    g_la, g_q = _out_arg(g_la, t[0]), _out_arg(g_q, t[3])
    stats = _stats_arg(stats, len(MPO_STATS), t[0].device)
    L.check(L.load().jh_mpo_loss_discrete(L.ctx(_dev(t[0])), R, int(T), A, *(L.ptr(v) for v in t), *(L.ptr(v) for v in cols), L.ptr(block), hyper_ptr, float(gamma),
                                          int(bool(retrace)), L.ptr(g_la), L.ptr(g_q), L.ptr(stats), L.stream_ptr()))
    return g_la, g_q, stats


MPO_MAX_ROWS, MPO_MAX_SAMPLED, MPO_MAX_CONT_ACTIONS = 1024, 8192, 8  # the caps of jh_mpo_sample / jh_mpo_loss_continuous: R, N * R, A


def mpo_sample(head_next, head_old, eps, out=None):
    """jh_mpo_sample: the raw Gaussian heads [mu | log_std] of online(s') and target(s), each [R, 2A], and standard normals eps [2, N, R, A].
    out = (z [2, N, R, A], a [2, N, R, A]) to write into.  -> (zn, zt_add, a_next, a_add), each [N, R, A]: views of the two."""
    hn, ho, eps = _f32(head_next), _f32(head_old), _f32(eps)
    two, N, R, A = eps.shape
    assert two == 2 and tuple(hn.shape) == tuple(ho.shape) == (R, 2 * A)
    z, a = out if out is not None else (torch.empty_like(eps), torch.empty_like(eps))
    assert all(t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (2, N, R, A) for t in (z, a))
    L.check(L.load().jh_mpo_sample(L.ctx(_dev(eps)), R, N, A, L.ptr(hn), L.ptr(ho), L.ptr(eps), L.ptr(z[0]), L.ptr(z[1]), L.ptr(a[0]), L.ptr(a[1]), L.stream_ptr()))
    return z[0], z[1], a[0], a[1]


def mpo_loss_continuous(head, head_old, q, qt_a, qt_next, qt_add, zt_add, action, reward, done, prob_b, T, block, hyper, gamma, retrace=True, stats=None, out=None):
    """jh_mpo_loss_continuous: the raw heads [R, 2A] of online(s) and target(s), the critic's online q and target qt_a [R], the target critic over
    the sampled actions qt_next / qt_add [N, R], zt_add [N, R, A], the stored action [R, A] and the replayed columns [R]; `block` and `hyper` as
    mpo_loss_discrete (all three multipliers are advanced).  out = (grad_head, grad_q) to write into.
    -> (grad_head [R, 2A], grad_q [R], stats f32[11] in the order of MPO_STATS)."""
    h, ho, zt, act = _f32(head), _f32(head_old), _f32(zt_add), _f32(action)
    N, R, A = zt.shape
    assert tuple(h.shape) == tuple(ho.shape) == (R, 2 * A) and act.numel() == R * A
    qn, qa = _f32(qt_next).reshape(N, -1), _f32(qt_add).reshape(N, -1)
    assert tuple(qn.shape) == tuple(qa.shape) == (N, R)
    cols = [_f32(v).reshape(-1) for v in (reward, done, prob_b)]
    q, qt_a = _f32(q).reshape(-1), _f32(qt_a).reshape(-1)
    assert all(v.numel() == R for v in cols + [q, qt_a])
    hyper_ptr = _mult_args(block, hyper, h.device)
    g_h, g_q = out if out is not None else (None, None)
    g_h, g_q = _out_arg(g_h, h), _out_arg(g_q, q)
    stats = _stats_arg(stats, len(MPO_STATS), h.device)
    L.check(L.load().jh_mpo_loss_continuous(L.ctx(_dev(h)), R, int(T), N, A, L.ptr(h), L.ptr(ho), L.ptr(q), L.ptr(qt_a), L.ptr(qn), L.ptr(qa), L.ptr(zt), L.ptr(act),
                                            *(L.ptr(v) for v in cols), L.ptr(block), hyper_ptr, float(gamma), int(bool(retrace)), L.ptr(g_h), L.ptr(g_q),
                                            L.ptr(stats), L.stream_ptr()))
    return g_h, g_q, stats


# ============================================================================= REINFORCE
REINFORCE_MAX_ROWS = 65536  # JH_REINFORCE_MAX_ROWS: the rows of one episode that one learn() takes
REINFORCE_STATS = ("loss", "rows")


def reinforce_returns(reward, gamma, standardize=True, out=None, T=None):
    """jh_reinforce_returns: reward [T] -> ret [T] float32, ret[t] = reward[t] + gamma ret[t + 1] over all T rows, then (standardize) the
    population standardisation, both in double on the device.  T: the row count handed to the library (default: reward's)."""
    r = _f32(reward).reshape(-1)
    T = int(r.numel()) if T is None else int(T)
    if out is None:
        out = torch.empty(max(T, 1), dtype=torch.float32, device=r.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= min(T, r.numel())
    L.check(L.load().jh_reinforce_returns(L.ctx(_dev(r)), T, L.ptr(r), float(gamma), int(bool(standardize)), L.ptr(out), L.stream_ptr()))
    return out


def _reinforce_loss(entry, head, A, action, ret, stats, out, T):
    h = _f32(head)
    T = int(h.shape[0]) if T is None else int(T)
    a, r = _f32(action).reshape(-1), _f32(ret).reshape(-1)
    grad = _out_arg(out, h, at_least=True)
    stats = _stats_arg(stats, len(REINFORCE_STATS), h.device)
    L.check(getattr(L.load(), entry)(L.ctx(_dev(h)), T, int(A), L.ptr(h), L.ptr(a), L.ptr(r), L.ptr(grad), L.ptr(stats), L.stream_ptr()))
    return grad, stats


def reinforce_loss_discrete(logits, action, ret, stats=None, out=None, T=None):
    """jh_reinforce_loss_discrete: logits [T, A], action [T] (any dtype, taken as float), ret [T] -> (d(loss)/d(logits) [T, A], stats f32[2] =
    {loss, T}) with loss = -mean_t(log_softmax(logits)[t, a_t] ret[t]).  Nothing is read back."""
    h = _f32(logits)
    assert h.dim() == 2 and (T is not None or (action.numel() == h.shape[0] and ret.numel() == h.shape[0]))
    return _reinforce_loss("jh_reinforce_loss_discrete", h, h.shape[1], action, ret, stats, out, T)


def reinforce_loss_continuous(head, action, ret, stats=None, out=None, T=None):
    """jh_reinforce_loss_continuous: head [T, 2A] = [mu_raw | log_std_raw], action [T, A], ret [T] -> (d(loss)/d(head) [T, 2A], stats f32[2] =
    {loss, T}) with loss = -mean over T * A of Normal(clamp(mu_raw, -5, 5), exp(tanh(log_std_raw))).log_prob(atanh(clamp(action))) ret[t]."""
    h = _f32(head)
    assert h.dim() == 2 and h.shape[1] % 2 == 0 and (T is not None or (action.numel() * 2 == h.numel() and ret.numel() == h.shape[0]))
    return _reinforce_loss("jh_reinforce_loss_continuous", h, h.shape[1] // 2, action, ret, stats, out, T)


# ============================================================================= R2D2
def lstm_step(groups, want_gates=False):
    """jh_lstm_step: one time step of torch.nn.LSTM for up to four row groups in ONE launch.  groups: a list of
    (xproj [R, 4H] -- rows may be strided --, w_hh [4H, H], h_prev [R, H], c_prev [R, H]); a group with R = 0 is skipped.
    -> a list of (h [R, H], c [R, H], gates [R, 4H] | None), the gates activated in the order i, f, g, o."""
    assert 1 <= len(groups) <= 4
    H = int(groups[0][1].shape[1])
    segs, outs = (L.LstmSeg * len(groups))(), []
    for s, (xp, w, h0, c0) in enumerate(groups):
        R = int(xp.shape[0])
        w, h0, c0 = _f32(w), _f32(h0), _f32(c0)
        assert xp.dtype == torch.float32 and xp.is_cuda and xp.shape[1] == 4 * H and xp.stride(1) == 1
        assert tuple(w.shape) == (4 * H, H) and tuple(h0.shape) == (R, H) and tuple(c0.shape) == (R, H)
        h, c = torch.empty_like(h0), torch.empty_like(c0)
        gates = torch.empty(R, 4 * H, dtype=torch.float32, device=h0.device) if want_gates else None
        segs[s] = L.LstmSeg(R, int(xp.stride(0)) if R > 1 else 4 * H, xp.data_ptr(), w.data_ptr(), h0.data_ptr(), c0.data_ptr(), h.data_ptr(), c.data_ptr(),
                            gates.data_ptr() if want_gates else None)
        outs.append((h, c, gates, (xp, w, h0, c0)))
    L.check(L.load().jh_lstm_step(L.ctx(_dev(groups[0][1])), H, len(groups), C.cast(segs, C.c_void_p), L.stream_ptr()))
    return [o[:3] for o in outs]


def lstm_step_backward(w_hh, gates, c_prev, c, dh_ext=None, dc_in=None, dgates_next=None):
    """jh_lstm_step_backward: dh_t = dh_ext + dgates_next @ w_hh, then the gradient of step t's pre-activation gates and dc_{t-1}.
    gates [R, 4H] activated (lstm_step's), c_prev / c [R, H]; dh_ext / dc_in [R, H] and dgates_next [R, 4H] may be None (zero).
    -> (dgates [R, 4H], dc_prev [R, H])."""
    w, g, c0, c1 = _f32(w_hh), _f32(gates), _f32(c_prev), _f32(c)
    R, H = (int(v) for v in c1.shape)
    assert tuple(w.shape) == (4 * H, H) and tuple(g.shape) == (R, 4 * H) and tuple(c0.shape) == (R, H)
    opt = [None if v is None else _f32(v) for v in (dgates_next, dh_ext, dc_in)]
    assert all(v is None or tuple(v.shape) == s for v, s in zip(opt, ((R, 4 * H), (R, H), (R, H))))
    dg, dc = torch.empty_like(g), torch.empty_like(c1)
    L.check(L.load().jh_lstm_step_backward(L.ctx(_dev(w)), R, H, L.ptr(opt[0]), L.ptr(w), L.ptr(opt[1]), L.ptr(opt[2]), L.ptr(g), L.ptr(c0), L.ptr(c1), L.ptr(dg),
                                           L.ptr(dc), L.stream_ptr()))
    return dg, dc


def r2d2_loss(q, next_q, next_target_q, action, reward, done, weights, n_burn_in, n_step, gamma, eta, alpha, eps=1e-3, stats=None, want_td=False):
    """jh_r2d2_loss (r2d2.py:113-159): q / next_q / next_target_q [T, B, A] time-major over the T = seq_len - n_burn_in trained steps;
    action / reward / done [B, seq_len + n_step - 1] (or [.., 1]) as the replay row holds them; weights [B].
    -> (grad_q [T, B, A], priority float64 [B], stats f32[8] = {loss, max_Q, 0, 0, 0, mark, 0, mark}, td [B, T] | None)."""
    t = [_f32(v) for v in (q, next_q, next_target_q)]
    T, B, A = (int(v) for v in t[0].shape)
    assert all(tuple(v.shape) == (T, B, A) for v in t)
    cols = [_f32(v).reshape(B, -1) for v in (action, reward, done)]
    assert all(v.shape[1] == T + int(n_burn_in) + int(n_step) - 1 for v in cols)
    w = _f32(weights).reshape(-1)
    assert w.numel() == B
    g = torch.empty_like(t[0])
    prio = torch.empty(B, dtype=torch.float64, device=g.device)
    td = torch.empty(B, T, dtype=torch.float32, device=g.device) if want_td else None
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=g.device)
    assert stats.dtype == torch.float32 and stats.numel() >= 8 and stats.is_contiguous()
    L.check(L.load().jh_r2d2_loss(L.ctx(_dev(g)), B, T, A, int(n_burn_in), int(n_step), *(L.ptr(v) for v in t), *(L.ptr(v) for v in cols), L.ptr(w), float(gamma),
                                  float(eta), float(alpha), float(eps), L.ptr(g), L.ptr(prio), L.ptr(td), L.ptr(stats), L.stream_ptr()))
    return g, prio, stats, td


# ============================================================================= native policy-value MLP
class _PinnedBlock:
    """One jh_pinned_alloc allocation, freed when the last reference goes: a PinnedBuffer and the holder of its device alias
    each keep one, neither keeps the other (no reference cycle, so plain reference counting releases the block)."""

    def __init__(self, device_index, nbytes):
        self.lib = L.load()
        self.host, self.dev = C.c_void_p(), C.c_void_p()
        L.check(self.lib.jh_pinned_alloc(L.ctx(device_index), nbytes, C.byref(self.host), C.byref(self.dev)))

    def __del__(self):
        try:
            if getattr(self, "host", None):
                self.lib.jh_pinned_free(self.host)
                self.host = None
        except Exception:
            pass


STATS_WAIT_S, ACT_WAIT_S = 2.0, 5.0  # bounds of PinnedBuffer.wait: learn() statistics, per-env-step actions


class PinnedBuffer:
    """Pinned host memory mapped into the device address space (jh_pinned_alloc), zero-filled: `.np` is the host view, `.dev` the
    CUDA tensor aliasing it for the kernels, `.dev_ptr` its raw device address.

    Small results come back through it without a D2H copy or a hipStreamSynchronize wake-up: the host arms the elements that the
    finishing kernel writes last (behind a system-scope fence) with a sentinel BEFORE it enqueues the launch, and waits for the
    sentinels to go; everything it enqueues meanwhile is stream-ordered behind that kernel.  float32 buffers: sentinel -1.0 at the
    marks (values that are never -1).  int64 buffers: -1 (actions are >= 0), the mark is the low 32-bit word of each element."""

    def __init__(self, shape, dtype, device=None):
        dtype = np.dtype(dtype)
        device = device if isinstance(device, torch.device) else torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        count = int(np.prod(shape))
        nbytes = max(count * dtype.itemsize, 8)
        self._block = _PinnedBlock(device.index, nbytes)
        self.dev_ptr = C.c_void_p(self._block.dev.value)
        self.np = np.frombuffer((C.c_char * nbytes).from_address(self._block.host.value), dtype=dtype, count=count).reshape(shape)
        self.np[...] = 0
        self.dev = _wrap_device(self._block.dev.value, shape, _TORCH_OF[_NP_DT[dtype]], device, owner=self._block)
        self._flat = self.np.reshape(-1)
        if dtype == np.int64:
            self._wait_fn, self._base, self._sentinel = self._block.lib.jh_host_wait_words, self._flat.view(np.uint32), 0xFFFFFFFF
        else:
            self._wait_fn, self._base, self._sentinel = self._block.lib.jh_host_wait_marks, self._flat, -1.0
        self._waits = {}  # marks -> (elements, pointer to _base, their int32 indices into _base, pointer to those, count): wait() is a per-env-step path

    def arm(self, marks=None):
        """Write the sentinel at the flat element indices `marks` (None: every element), before the launch that overwrites them."""
        if marks is None:
            self._flat.fill(-1)
        else:
            for m in marks:
                self._flat[m] = -1

    def wait(self, marks=None, what="PinnedBuffer.wait(): the results", stream=None, timeout_s=STATS_WAIT_S):
        """Wait until no element of `marks` (as armed) holds the sentinel.  One ctypes call: a C spin, i.e. without the GIL (a Python spin
        loop here cost the batched actors of an Ape-X process a third of their throughput).  Bounded: after `timeout_s` a synchronise
        of `stream` (default: torch's current stream of the buffer's device), which also surfaces asynchronous errors, then an error if
        the marks are still there."""
        w = self._waits.get(marks)
        if w is None:
            assert self.np.dtype in (np.float32, np.int64), "arrival marks are float32 elements or the low words of int64 elements"
            el = np.arange(self._flat.size, dtype=np.int32) if marks is None else np.asarray(marks, dtype=np.int32)
            idx = el * (self._base.size // self._flat.size)  # int64: the low word (little endian) of each element
            w = self._waits[marks] = (el, L.ptr(self._base), idx, L.ptr(idx), int(idx.size))
        if self._wait_fn(w[1], w[3], w[4], self._sentinel, timeout_s) != 0:
            (torch.cuda.current_stream(self.dev.device) if stream is None else stream).synchronize()
            if (self._flat[w[0]] == -1).any():
                raise RuntimeError(f"{what} never arrived (failed launch?)")


class PPONet:
    """jh_pponet_*: S -> H relu -> H relu -> heads, fwd / bwd / clip + Adam on flat fp32 buckets."""

    def __init__(self, S, H, A, continuous, max_rows, device, seed=0):
        self.lib = L.load()
        self.device = torch.device(device)
        self.ctx = L.ctx(self.device.index)
        self.S, self.H, self.A, self.cont, self.max_rows = int(S), int(H), int(A), bool(continuous), int(max_rows)
        self.n_params = int(self.lib.jh_pponet_param_count(self.S, self.H, self.A, int(self.cont)))
        mk = lambda: torch.zeros(self.n_params, dtype=torch.float32, device=self.device)
        self.params, self.grads, self.m, self.v = mk(), mk(), mk(), mk()
        self.h = C.c_void_p()
        L.check(self.lib.jh_pponet_create(self.ctx, self.S, self.H, self.A, int(self.cont), self.max_rows, L.ptr(self.params), L.ptr(self.grads), L.ptr(self.m), L.ptr(self.v), C.c_uint64(int(seed)), C.byref(self.h)))
        self._act = None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_pponet_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=-1.0):
        """step >= 0 sets Adam's step counter (0 = fresh optimizer), step < 0 keeps it."""
        L.check(self.lib.jh_pponet_set_hyper(self.h, float(lr), float(beta1), float(beta2), float(eps), float(step), L.stream_ptr()))

    def set_lr(self, lr):
        L.check(self.lib.jh_pponet_set_lr(self.h, float(lr), L.stream_ptr()))

    def hyper_ptr(self):
        return int(self.lib.jh_pponet_hyper_ptr(self.h))

    def act_rng(self, state=None):
        """(seed, counter) of the host-side sampling stream; state=(seed, counter) restores it."""
        s, c = C.c_uint64(0), C.c_uint64(0)
        if state is not None:
            s, c = C.c_uint64(int(state[0])), C.c_uint64(int(state[1]))
        L.check(self.lib.jh_pponet_act_rng(self.h, C.byref(s), C.byref(c), int(state is not None)))
        return int(s.value), int(c.value)

    def forward(self, x, idx=None, B=None, out=None):
        """x float32 [*, S]; rows gathered by idx (int64 [B]) when given.  Returns raw heads
        (logits, value) or (mu_raw, log_std_raw, value); `out` = preallocated tuple."""
        B = int(idx.numel()) if idx is not None else (int(x.shape[0]) if B is None else int(B))
        if out is None:
            h0 = torch.empty(B, self.A, dtype=torch.float32, device=self.device)
            h1 = torch.empty(B, self.A, dtype=torch.float32, device=self.device) if self.cont else None
            val = torch.empty(B, 1, dtype=torch.float32, device=self.device)
        else:
            h0, h1, val = out
        flops = 2.0 * B * self.H * (self.S + self.H + (2 * self.A + 1 if self.cont else self.A + 1))
        with _timed("jh_pponet_forward", flops, "mfma"):
            L.check(self.lib.jh_pponet_forward(self.h, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(h0), L.ptr(h1), L.ptr(val), L.stream_ptr()))
        return (h0, h1, val) if self.cont else (h0, val)

    def backward(self, x, idx, g_head0, g_head1, g_value, B=None):
        B = int(idx.numel()) if idx is not None else (int(x.shape[0]) if B is None else int(B))
        flops = 4.0 * B * self.H * (self.S + self.H + (2 * self.A + 1 if self.cont else self.A + 1))
        with _timed("jh_pponet_backward", flops, "mfma"):
            L.check(self.lib.jh_pponet_backward(self.h, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(g_head0), L.ptr(g_head1), L.ptr(g_value), L.stream_ptr()))

    def adam_step(self, max_norm, norm_out=None):
        with _timed("jh_gradnorm+adam", 4.0 * self.n_params * 8):  # g (r twice, w) + p,m,v (r+w)
            L.check(self.lib.jh_pponet_adam_step(self.h, float(max_norm if max_norm else 0.0), L.ptr(norm_out), L.stream_ptr()))

    def fused_ok(self, B):
        """Minibatches the four- / five-launch update (jh_pponet_ppo_update) takes: < 1024 rows (from there on the
        LDS-tiled engine wins), hidden width a multiple of 32."""
        n_out = (2 * self.A + 1) if self.cont else (self.A + 1)
        return self.H % 32 == 0 and 0 < B < 1024 and n_out <= 8  # wider heads (round 5): the separate forward / loss / backward / Adam calls

    def ppo_update(self, x, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, max_norm, stats, do_adam=True):
        """One whole PPO minibatch update in 4 launches (5 beyond 256 rows or with do_adam=False) (jh_pponet_ppo_update).  B = idx.numel() <= 1024."""
        B = int(idx.numel()) if idx is not None else int(x.shape[0])
        L.check(self.lib.jh_pponet_ppo_update(self.h, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(_f32(action)), L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)),
                                              L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(logp_old)), float(eps_clip), float(vf_coef), float(ent_coef),
                                              float(max_norm if max_norm else 0.0), int(bool(do_adam)), L.ptr(stats), L.stream_ptr()))

    def ppo_update_rows(self, x, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, max_norm, stats, do_adam=True):
        """The same update for any B <= max_rows in one call (jh_pponet_ppo_update_rows): forward, the loss forward + backward in ONE launch, backward,
        [clip + Adam].  What minibatches of >= 1024 rows / nets with more than 8 head outputs take; bit-identical to forward -> ppo_loss_* -> backward -> adam_step."""
        B = int(idx.numel()) if idx is not None else int(x.shape[0])
        L.check(self.lib.jh_pponet_ppo_update_rows(self.h, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(_f32(action)), L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)),
                                                   L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(logp_old)), float(eps_clip), float(vf_coef), float(ent_coef),
                                                   float(max_norm if max_norm else 0.0), int(bool(do_adam)), L.ptr(stats), L.stream_ptr()))

    def ppo_update_dp(self, x, idx, action, adv, ret, value_old, logp_old, eps_clip, vf_coef, ent_coef, stats, reduce_mean, critic_sums, peer=None):
        """The minibatch update for data-parallel learners with the reference's critic exactly (jh_pponet_ppo_update_dp_begin / _end around
        an 8-byte all-reduce): reduce_mean(t) all-reduces a small fp32 device tensor to its mean over the ranks, in place, on the current
        stream.  Leaves a complete gradient bucket; the caller reduces it and calls adam_step."""
        B = int(idx.numel()) if idx is not None else int(x.shape[0])
        L.check(self.lib.jh_pponet_ppo_update_dp_begin(self.h, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(_f32(action)), L.ptr(_f32(adv).reshape(-1)), L.ptr(_f32(ret).reshape(-1)),
                                                       L.ptr(_f32(value_old).reshape(-1)), L.ptr(_f32(logp_old)), float(eps_clip), float(vf_coef), float(ent_coef),
                                                       L.ptr(critic_sums), L.stream_ptr()))
        if peer is not None and B <= 256:  # peer-pointer transport: the ranks' sums meet inside the second half's first launch
            L.check(self.lib.jh_pponet_ppo_update_dp_end_peer(self.h, peer, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(critic_sums), float(vf_coef), float(ent_coef), L.ptr(stats), L.stream_ptr()))
            return
        reduce_mean(critic_sums)
        L.check(self.lib.jh_pponet_ppo_update_dp_end(self.h, B, L.ptr(_f32(x)), L.ptr(idx), L.ptr(critic_sums), float(vf_coef), float(ent_coef), L.ptr(stats), L.stream_ptr()))

    # ---- acting (one launch; partial heads come back through device-mapped pinned memory) ---------
    def act_discrete(self, obs, training=True, want_logits=False):
        """obs: numpy float32 [W, S] -> numpy int64 [W, 1] (blocking)."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        W = int(obs.shape[0])
        act = np.empty((W, 1), np.int64)
        logits = np.empty((W, self.A), np.float32) if want_logits else None
        val = np.empty((W, 1), np.float32) if want_logits else None
        L.check(self.lib.jh_pponet_act_discrete(self.h, W, L.ptr(obs), L.ptr(act), L.ptr(logits), L.ptr(val), int(bool(training)), L.stream_ptr()))
        return (act, logits, val) if want_logits else act


class NormalSource:
    """jh_normal_fill: N(0,1) draws on the device from a counter-based generator whose call counter lives in device
    memory (a replayed hipGraph draws fresh noise).  fill(t) overwrites the float32 CUDA tensor t in place."""

    def __init__(self, device, seed=None):
        self.lib = L.load()
        self.device = torch.device(device)
        self.ctx = L.ctx(self.device.index)
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())  # tied to torch.manual_seed
        self.state = torch.tensor([int(seed), 0, 0, 0], dtype=torch.int64, device=self.device)

    def fill(self, t):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        L.check(self.lib.jh_normal_fill(self.ctx, int(t.numel()), L.ptr(t), L.ptr(self.state), L.stream_ptr()))
        return t


def _act_buffers(R, A, dev, eps, u, rand_action, out, want_q_all):
    """What value_act / quantile_act / iqn_act share: the outputs (act int64 [R] and q float32 [R], or the caller's `out` pair; q_all
    float32 [R, A] when wanted) and the three host draw arrays, contiguous in the types the library reads (or all None)."""
    act, q = (torch.empty(R, dtype=torch.int64, device=dev), torch.empty(R, dtype=torch.float32, device=dev)) if out is None else out
    q_all = torch.empty(R, A, dtype=torch.float32, device=dev) if want_q_all else None
    if eps is not None:
        eps, u, rand_action = (np.ascontiguousarray(eps, dtype=np.float32), np.ascontiguousarray(u, dtype=np.float64), np.ascontiguousarray(rand_action, dtype=np.int64))
        assert eps.size == R and u.size == R and rand_action.size == R
    return act, q, q_all, eps, u, rand_action


def value_act(logits, v_min=0.0, v_max=0.0, eps=None, u=None, rand_action=None, out=None, want_q_all=False):
    """jh_value_act: network outputs [N, A, K] (K = 1: Q values) -> (action int64 [N], q_taken float32 [N], q_all | None)
    on the device.  eps / u / rand_action: numpy float32 / float64 / int64 [N] (the host's epsilon-greedy draws) or
    all None for greedy."""
    lg = _f32(logits)
    N, A, K = (int(v) for v in lg.shape)
    act, q, q_all, eps, u, rand_action = _act_buffers(N, A, lg.device, eps, u, rand_action, out, want_q_all)
    L.check(L.load().jh_value_act(L.ctx(_dev(lg)), N, A, K, L.ptr(lg), float(v_min), float(v_max), L.ptr(eps), L.ptr(u), L.ptr(rand_action), L.ptr(act), L.ptr(q),
                                  L.ptr(q_all), L.stream_ptr()))
    return act, q, q_all


def _pponet_act_continuous(self, obs, training=True, want_heads=False):
    """obs: numpy float32 [W, S] -> numpy float32 [W, A] in (-1, 1) (blocking); PPO.act, ppo.py:55-63."""
    obs = np.ascontiguousarray(obs, dtype=np.float32)
    W = int(obs.shape[0])
    act = np.empty((W, self.A), np.float32)
    mu = np.empty((W, self.A), np.float32) if want_heads else None
    ls = np.empty((W, self.A), np.float32) if want_heads else None
    L.check(self.lib.jh_pponet_act_continuous(self.h, W, L.ptr(obs), L.ptr(act), L.ptr(mu), L.ptr(ls), None, int(bool(training)), L.stream_ptr()))
    return (act, mu, ls) if want_heads else act


PPONet.act_continuous = _pponet_act_continuous


# ============================================================================= TD / C51
def td_loss(q, q_next_target, action, reward, done, gamma, q_next_online=None, weights=None, alpha=0.0, n_step=0, stats=None):
    """Returns (grad_q [B,A], prio [B], stats f32[4] = {loss, max_Q, mean_td, 0})."""
    lib = L.load()
    q = _f32(q)
    B, A = q.shape
    flags = (L.JH_TD_DOUBLE if q_next_online is not None else 0) | (L.JH_TD_PER if weights is not None else 0)
    g = torch.empty_like(q)
    prio = torch.empty(B, dtype=torch.float32, device=q.device)
    if stats is None:
        stats = torch.empty(4, dtype=torch.float32, device=q.device)
    r, d = _f32(reward).reshape(B, -1), _f32(done).reshape(B, -1)
    assert r.shape[1] == max(n_step, 1) and d.shape == r.shape
    L.check(lib.jh_td_loss(L.ctx(_dev(q)), B, A, int(n_step), flags, L.ptr(q), L.ptr(None if q_next_online is None else _f32(q_next_online)), L.ptr(_f32(q_next_target)), L.ptr(_f32(action).reshape(-1)), L.ptr(r), L.ptr(d), L.ptr(None if weights is None else _f32(weights).reshape(-1)), float(gamma), float(alpha), L.ptr(g), L.ptr(prio), L.ptr(stats), L.stream_ptr()))
    return g, prio, stats


@contextlib.contextmanager
def graph_capture(g):
    """`with torch.cuda.graph(g, capture_error_mode="thread_local")` plus the two things this torch build leaves to the caller:

    * garbage collection.  torch.cuda.graph.__enter__ only collects when torch.compiler.config.force_cudagraph_gc is set (it is not): a dead
      reference cycle left by an EARLIER agent (agent <-> collector, owning device buffers, pinned memory, events) is then finalized by
      whichever Python allocation happens to trip the cyclic collector -- and if that is one inside the capture, the hipFree / hipHostFree /
      hipEventDestroy comes from the capturing thread and invalidates the capture (hipErrorStreamCaptureInvalidated at the next launch;
      seen in ~1 of 8 runs of the GPU suite, always in a test that follows many agent + collector pairs, never in that test alone).
      So: one full collection in front, the automatic collector off while capturing.
    * a failed capture.  torch.cuda.graph.__exit__ raises out of capture_end() BEFORE it restores the stream: the capture stream -- torch's
      process-wide default one -- stays current and stays capturing, and everything enqueued afterwards fails.  Here the previous stream
      is made current again, the abandoned capture is ended, and torch is given a fresh default capture stream; the caller's eager
      fallback then runs on a healthy stream."""
    import gc

    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    prev = torch.cuda.current_stream()
    cm = torch.cuda.graph(g, capture_error_mode="thread_local")  # other threads (batched actors, staging ring, collector) keep issuing HIP work on their own streams
    try:
        with cm:
            yield
    except BaseException:
        try:
            torch.cuda.set_stream(prev)
            L.load().jh_stream_abort_capture(C.c_void_p(cm.capture_stream.cuda_stream))
            if torch.cuda.graph.default_capture_stream is cm.capture_stream:
                torch.cuda.graph.default_capture_stream = None
        except Exception:
            pass
        raise
    finally:
        if was_enabled:
            gc.enable()


class LearnGraphs:
    """The hipGraph lifecycle of an agent's learn(), the same for every agent: a body runs eagerly the first time (that warms it), is
    captured the next time it is eligible, and is replayed from then on.  A capture that raises (e.g. a collective that refuses capture)
    is synchronised away and reported once, and the agent stays eager for good.  A captured graph holds the addresses of the static
    buffers it was captured on: whoever replaces them calls reset()."""

    def __init__(self, what):
        self.what, self.graphs, self.warm, self.failed, self.last = what, {}, set(), False, None  # last: the graph most recently replayed

    def reset(self):
        """Drop the graphs; what has run eagerly once stays warm."""
        self.graphs.clear()
        self.last = None

    def ready(self, key, bodies, eligible, warm_key, capture=True):
        """May this call replay `key`?  First captures `bodies` ({key: body}; those not held yet, all or none) when that is due: `key` is
        eligible, warm and not captured, and `capture` is on (a capture synchronises the device; a caller that cannot have that now
        still replays what it holds)."""
        usable = eligible and not self.failed and not _PROF["lib"]
        if usable and capture and key not in self.graphs and warm_key in self.warm:
            try:
                new = {}
                torch.cuda.synchronize()
                for k, body in bodies.items():
                    if k not in self.graphs:
                        new[k] = torch.cuda.CUDAGraph()
                        with graph_capture(new[k]):  # capture does not execute: the replay that follows runs this call's update
                            body()
                self.graphs.update(new)
            except Exception as e:
                self.reset()
                self.failed = True
                torch.cuda.synchronize()
                print(f"[jorldy_amd] hipGraph capture of {self.what} failed ({type(e).__name__}: {e}); running eagerly")
                return False
        return bool(usable and key in self.graphs)

    def replay(self, key):
        self.last = self.graphs[key]
        self.last.replay()

    def run(self, key, body, eligible=True, warm_key=None):
        """Run `body` eagerly, or capture it and / or replay its graph; -> was it a replay.  `warm_key`: what the eager run warms and a
        capture waits for (default: `key` itself; variants that share one warm-up pass one name)."""
        warm_key = key if warm_key is None else warm_key
        if self.ready(key, {key: body}, eligible, warm_key):
            self.replay(key)
            return True
        body()
        self.warm.add(warm_key)
        return False


def c51_loss(logit, target_logit, action, reward, done, v_min, v_max, gamma, next_logit_online=None, weights=None, alpha=0.0, n_step=0, shift_max=False, stats=None):
    """logit/target_logit/next_logit_online [B,A,K].  Returns (grad_logit, prio [B], kl [B], stats f32[8])."""
    lib = L.load()
    z = _f32(logit)
    B, A, K = z.shape
    flags = (L.JH_C51_DOUBLE if next_logit_online is not None else 0) | (L.JH_C51_PER if weights is not None else 0) | (L.JH_C51_SHIFT_MAX if shift_max else 0)
    g = torch.empty_like(z)
    prio = torch.empty(B, dtype=torch.float32, device=z.device)
    kl = torch.empty(B, dtype=torch.float32, device=z.device)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=z.device)
    r, d = _f32(reward).reshape(B, -1), _f32(done).reshape(B, -1)
    assert r.shape[1] == max(n_step, 1) and d.shape == r.shape
    L.check(lib.jh_c51_loss(L.ctx(_dev(z)), B, A, K, int(n_step), flags, L.ptr(z), L.ptr(None if next_logit_online is None else _f32(next_logit_online)), L.ptr(_f32(target_logit)), L.ptr(_f32(action).reshape(-1)), L.ptr(r), L.ptr(d), L.ptr(None if weights is None else _f32(weights).reshape(-1)), float(v_min), float(v_max), float(gamma), float(alpha), L.ptr(g), L.ptr(prio), L.ptr(kl), L.ptr(stats), L.stream_ptr()))
    return g, prio, kl, stats


def _quantile_loss(entry, B, A, N, z, next_logit_online, target_logit, action, reward, done, t, gamma, stats):
    """What qr_loss / iqn_loss share once the layout is read off `z`: the two other networks' outputs in z's shape, the [B] vectors
    flat, the gradient and the stats block allocated, the call."""
    zn, zt = _f32(next_logit_online), _f32(target_logit)
    assert zn.shape == z.shape and zt.shape == z.shape and t.device == z.device
    a, r, d = _f32(action).reshape(-1), _f32(reward).reshape(-1), _f32(done).reshape(-1)
    assert a.numel() == B and r.numel() == B and d.numel() == B
    g = torch.empty_like(z)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=z.device)
    L.check(entry(L.ctx(_dev(z)), B, A, N, L.ptr(z), L.ptr(zn), L.ptr(zt), L.ptr(a), L.ptr(r), L.ptr(d), L.ptr(t), float(gamma), L.ptr(g), L.ptr(stats), L.stream_ptr()))
    return g, stats


def qr_loss(logit, next_logit_online, target_logit, action, reward, done, tau, gamma, stats=None):
    """jh_qr_loss (qrdqn.py:60-95): logit / next_logit_online / target_logit [B, A, N], action / reward / done [B] (or [B, 1]),
    tau float32 [N] on the device.  Returns (grad_logit [B, A, N], stats f32[8] = {loss, max_Q, max_logit, min_logit, 0, mark, 0, mark})."""
    z, t = _f32(logit), _f32(tau).reshape(-1)
    B, A, N = (int(v) for v in z.shape)
    assert t.numel() == N
    return _quantile_loss(L.load().jh_qr_loss, B, A, N, z, next_logit_online, target_logit, action, reward, done, t, gamma, stats)


def mdqn_loss(q, q_target, q_next_target, action, reward, done, gamma, alpha, tau, l_0, stats=None):
    """jh_mdqn_loss (m_dqn.py:29-59): q / q_target / q_next_target [B, A] = online(s), target(s), target(s'), action / reward / done [B]
    (or [B, 1]).  Returns (grad_q [B, A], stats f32[4] = {loss, max taken Q, mean Munchausen term, mark})."""
    q = _f32(q)
    B, A = (int(v) for v in q.shape)
    qt, qn = _f32(q_target), _f32(q_next_target)
    assert tuple(qt.shape) == (B, A) and tuple(qn.shape) == (B, A)
    a, r, d = _f32(action).reshape(-1), _f32(reward).reshape(-1), _f32(done).reshape(-1)
    assert a.numel() == B and r.numel() == B and d.numel() == B
    g = torch.empty_like(q)
    if stats is None:
        stats = torch.empty(4, dtype=torch.float32, device=q.device)
    L.check(L.load().jh_mdqn_loss(L.ctx(_dev(q)), B, A, L.ptr(q), L.ptr(qt), L.ptr(qn), L.ptr(a), L.ptr(r), L.ptr(d), float(gamma), float(alpha), float(tau), float(l_0),
                                  L.ptr(g), L.ptr(stats), L.stream_ptr()))
    return g, stats


def quantile_act(logits, eps=None, u=None, rand_action=None, out=None, want_q_all=False):
    """jh_quantile_act: network outputs [R, A, N] (N quantiles per action, Q = their mean) -> (action int64 [R], q_taken float32 [R],
    q_all | None) on the device.  eps / u / rand_action as in value_act."""
    lg = _f32(logits)
    R, A, N = (int(v) for v in lg.shape)
    act, q, q_all, eps, u, rand_action = _act_buffers(R, A, lg.device, eps, u, rand_action, out, want_q_all)
    L.check(L.load().jh_quantile_act(L.ctx(_dev(lg)), R, A, N, L.ptr(lg), L.ptr(eps), L.ptr(u), L.ptr(rand_action), L.ptr(act), L.ptr(q), L.ptr(q_all), L.stream_ptr()))
    return act, q, q_all


def iqn_loss(logit, next_logit_online, target_logit, action, reward, done, tau, gamma, stats=None):
    """jh_iqn_loss (iqn.py:89-121): logit / next_logit_online / target_logit [B, N, A] as the network writes them, action / reward / done [B]
    (or [B, 1]), tau float32 [B, N] = the draw of the forward that produced `logit`.  Returns (grad_logit [B, N, A], stats f32[8] as qr_loss)."""
    z, t = _f32(logit), _f32(tau)
    B, N, A = (int(v) for v in z.shape)
    assert t.numel() == B * N
    return _quantile_loss(L.load().jh_iqn_loss, B, A, N, z, next_logit_online, target_logit, action, reward, done, t, gamma, stats)


def miqn_loss(logit, logit_again, target_logit, action, reward, done, tau, gamma, alpha, tau_e, l_0, stats=None):
    """jh_miqn_loss (m_iqn.py:29-95): logit / logit_again = online(state) under the first and a second draw, target_logit =
    target(next_state), each [B, N, A]; action / reward / done [B] (or [B, 1]); tau float32 [B, N] = the FIRST draw; tau_e the entropy
    temperature.  Returns (grad_logit [B, N, A], stats f32[8] as iqn_loss, max / min logit taken from logit_again)."""
    z, t = _f32(logit), _f32(tau)
    B, N, A = (int(v) for v in z.shape)
    assert t.numel() == B * N
    entry = lambda ctx, B, A, N, z, zn, zt, a, r, d, t, gamma, g, stats, stream: L.load().jh_miqn_loss(
        ctx, B, A, N, z, zn, zt, a, r, d, t, gamma, float(alpha), float(tau_e), float(l_0), g, stats, stream)
    return _quantile_loss(entry, B, A, N, z, logit_again, target_logit, action, reward, done, t, gamma, stats)


def riqn_loss(logit, next_logit_online, target_logit, action, reward, done, weights, tau, gamma, alpha, n_step, stats=None):
    """jh_riqn_loss (rainbow_iqn.py:158-224): iqn_loss's arguments with reward / done [B, n_step] (the stored window, folded from its last
    step to its first), the importance weights [B] and the priority exponent.  Returns (grad_logit [B, N, A], prio [B] = loss_b ^ alpha,
    stats f32[8] as iqn_loss with stats[0] = mean(w) * mean_b(loss_b), the reference's [B, 1] x [B] broadcast)."""
    z, t = _f32(logit), _f32(tau)
    B, N, A = (int(v) for v in z.shape)
    zn, zt = _f32(next_logit_online), _f32(target_logit)
    assert t.numel() == B * N and zn.shape == z.shape and zt.shape == z.shape and t.device == z.device
    a, w = _f32(action).reshape(-1), _f32(weights).reshape(-1)
    r, d = _f32(reward).reshape(B, -1), _f32(done).reshape(B, -1)
    assert a.numel() == B and w.numel() == B and r.shape[1] == max(int(n_step), 1) and d.shape == r.shape
    g = torch.empty_like(z)
    prio = torch.empty(B, dtype=torch.float32, device=z.device)
    if stats is None:
        stats = torch.empty(8, dtype=torch.float32, device=z.device)
    L.check(L.load().jh_riqn_loss(L.ctx(_dev(z)), B, A, N, int(n_step), L.ptr(z), L.ptr(zn), L.ptr(zt), L.ptr(a), L.ptr(r), L.ptr(d), L.ptr(w), L.ptr(t), float(gamma),
                                  float(alpha), L.ptr(g), L.ptr(prio), L.ptr(stats), L.stream_ptr()))
    return g, prio, stats


def iqn_act(logits, eps=None, u=None, rand_action=None, out=None, want_q_all=False):
    """jh_iqn_act: network outputs [R, N, A] (N samples per row, Q = their mean) -> (action int64 [R], q_taken float32 [R], q_all | None)
    on the device.  eps / u / rand_action as in value_act."""
    lg = _f32(logits)
    R, N, A = (int(v) for v in lg.shape)
    act, q, q_all, eps, u, rand_action = _act_buffers(R, A, lg.device, eps, u, rand_action, out, want_q_all)
    L.check(L.load().jh_iqn_act(L.ctx(_dev(lg)), R, A, N, L.ptr(lg), L.ptr(eps), L.ptr(u), L.ptr(rand_action), L.ptr(act), L.ptr(q), L.ptr(q_all), L.stream_ptr()))
    return act, q, q_all


def iqn_cos_features(tau, E):
    """jh_iqn_cos_features: tau float32 [...] -> cos(tau * (arange(E) * pi as float32)) [..., E], the argument rounded to float32 (iqn.py:14, 46)."""
    t = _f32(tau)
    out = torch.empty(tuple(t.shape) + (int(E),), dtype=torch.float32, device=t.device)
    L.check(L.load().jh_iqn_cos_features(L.ctx(_dev(t)), int(t.numel()), int(E), L.ptr(t), L.ptr(out), L.stream_ptr()))
    return out


def iqn_hadamard(psi, phi):
    """jh_iqn_hadamard: psi [B, H], phi [B, N, H] -> psi[:, None, :] * phi (iqn.py:34)."""
    p, f = _f32(psi), _f32(phi)
    B, N, H = (int(v) for v in f.shape)
    assert tuple(p.shape) == (B, H)
    out = torch.empty_like(f)
    L.check(L.load().jh_iqn_hadamard(L.ctx(_dev(f)), B, N, H, L.ptr(p), L.ptr(f), L.ptr(out), L.stream_ptr()))
    return out


def iqn_hadamard_backward(grad_embed, psi, phi):
    """jh_iqn_hadamard_backward: the product's backward through both relus -> (d phi_pre [B, N, H], d psi_pre [B, H]); psi / phi are the
    relu outputs of the forward."""
    g, p, f = _f32(grad_embed), _f32(psi), _f32(phi)
    B, N, H = (int(v) for v in f.shape)
    assert tuple(p.shape) == (B, H) and tuple(g.shape) == (B, N, H)
    dphi, dpsi = torch.empty_like(f), torch.empty_like(p)
    L.check(L.load().jh_iqn_hadamard_backward(L.ctx(_dev(f)), B, N, H, L.ptr(g), L.ptr(p), L.ptr(f), L.ptr(dphi), L.ptr(dpsi), L.stream_ptr()))
    return dphi, dpsi


# ============================================================================= host collector
class CartPoleVec:
    """W synthetic CartPole-v1 envs stepped in one native call (jh_cartpole_*)."""

    def __init__(self, W, seed=0):
        self.lib = L.load()
        self.W = int(W)
        self.h = C.c_void_p()
        L.check(self.lib.jh_cartpole_create(self.W, C.c_uint64(int(seed)), C.byref(self.h)))
        self.state_size, self.action_size, self.action_type = 4, 2, "discrete"

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_cartpole_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def obs(self, out=None):
        out = np.empty((self.W, 4), np.float32) if out is None else out
        L.check(self.lib.jh_cartpole_obs(self.h, L.ptr(out)))
        return out

    def step(self, action, next_obs=None, reward=None, done=None):
        a = np.ascontiguousarray(action, dtype=np.int64).reshape(-1)
        assert a.size == self.W
        next_obs = np.empty((self.W, 4), np.float32) if next_obs is None else next_obs
        reward = np.empty(self.W, np.float32) if reward is None else reward
        done = np.empty(self.W, np.uint8) if done is None else done
        L.check(self.lib.jh_cartpole_step(self.h, L.ptr(a), L.ptr(next_obs), L.ptr(reward), L.ptr(done)))
        return next_obs, reward, done


class ControlVec:
    """W synthetic continuous-control envs (jh_control_*: stand-in for MuJoCo at config.ppo.mujoco shapes, default
    Hopper-v3's S = 11, A = 3) stepped in one native call."""

    def __init__(self, W, state_size=11, action_size=3, seed=0):
        self.lib = L.load()
        self.W, self.state_size, self.action_size, self.action_type = int(W), int(state_size), int(action_size), "continuous"
        self.h = C.c_void_p()
        L.check(self.lib.jh_control_create(self.W, self.state_size, self.action_size, C.c_uint64(int(seed)), C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_control_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def obs(self, out=None):
        out = np.empty((self.W, self.state_size), np.float32) if out is None else out
        L.check(self.lib.jh_control_obs(self.h, L.ptr(out)))
        return out

    def step(self, action, next_obs=None, reward=None, done=None):
        a = np.ascontiguousarray(action, dtype=np.float32).reshape(self.W, self.action_size)
        next_obs = np.empty((self.W, self.state_size), np.float32) if next_obs is None else next_obs
        reward = np.empty(self.W, np.float32) if reward is None else reward
        done = np.empty(self.W, np.uint8) if done is None else done
        L.check(self.lib.jh_control_step(self.h, L.ptr(a), L.ptr(next_obs), L.ptr(reward), L.ptr(done)))
        return next_obs, reward, done


class _NetObject:
    """What RainbowNet, IQNNet and _ActorCriticBuckets share below their architecture: library / device / context, zeroed flat float32
    buckets, the segment table name -> (offset, rows, cols) read through the native entries `_SYM + name`, and destroy on collection."""

    def _open(self, device):
        self.lib = L.load()
        self.device = torch.device(device)
        self.ctx = L.ctx(self.device.index)

    def _fn(self, name):
        return getattr(self.lib, self._SYM + name)

    def _zeros(self, n, count=5):
        return [torch.zeros(n, dtype=torch.float32, device=self.device) for _ in range(count)]

    def _segments(self, names, first=0):
        seg = {}
        for i, name in enumerate(names, first):
            off, rows, cols = C.c_int64(), C.c_int32(), C.c_int32()
            L.check(self._fn("segment")(self.h, i, C.byref(off), C.byref(rows), C.byref(cols)))
            seg[name] = (off.value, rows.value, cols.value)
        return seg

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self._fn("destroy")(self.h)
                self.h = None
        except Exception:
            pass


def _seg_pairs(flat, seg):
    """[(name, view of its segment of `flat`: [rows, cols] for a .weight, flat otherwise)] in the table's order."""
    out = []
    for name, (off, rows, cols) in seg.items():
        v = flat[off : off + rows * cols]
        out.append((name, v.view(rows, cols) if name.endswith(".weight") else v))
    return out


def _export_pairs(pairs):
    from collections import OrderedDict

    return OrderedDict((k, v.clone(memory_format=torch.contiguous_format)) for k, v in pairs)


@torch.no_grad()
def _import_pairs(pairs, sd, device, shaped=lambda k, v, src: src):
    """Copy sd[k] into the view v for every (k, v); `shaped` may re-view a source before its shape is checked."""
    pairs = dict(pairs)
    missing = [k for k in pairs if k not in sd]
    if missing:
        raise KeyError(f"state_dict is missing {missing}")
    for k, v in pairs.items():
        src = shaped(k, v, torch.as_tensor(sd[k]).to(device, torch.float32))
        if tuple(src.shape) != tuple(v.shape):
            raise ValueError(f"{k}: expected {tuple(v.shape)}, got {tuple(src.shape)}")
        v.copy_(src)


class RainbowNet(_NetObject):
    """jh_rbnet_*: the value networks of the DQN / Rainbow / Ape-X family -- kind "rainbow" (MLP or Nature-CNN
    head -> Linear -> noisy dueling categorical heads), "dueling" (head -> l1_a|l1_v -> l2_a, l2_v) and "q"
    (head -> l -> q) -- with the three learn() forwards, backward and the optimizer step as grouped MFMA GEMM
    launches.

    Parameters live in flat fp32 buckets in the library's private layout; `export_state` / `import_state`
    convert to and from the reference's `state_dict` (network/{rainbow,dueling,q_network}.py key names, shapes
    and order), so checkpoints and sync_in / sync_out payloads interchange."""

    _SEG = ("w1", "b1", "w2", "b2", "w3", "b3", "wl", "bl", "mu_av1", "sig_av1", "mub_av1", "sigb_av1", "mu_a2", "sig_a2", "mub_a2", "sigb_a2",
            "mu_v2", "sig_v2", "mub_v2", "sigb_v2")
    _SYM = "jh_rbnet_"
    _KIND = {"rainbow": 0, "dueling": 1, "q": 2, "pv": 2, "pi": 2, "gauss": 2, "pv2": 2, "gauss2": 2, "noisy": 4}  # "noisy": network/noisy.py (head -> noisy -> noisy; 5 with independent noise); "pv": the discrete policy-value net (policy_value.py:8-22) = head -> l -> (pi | v) stacked into ONE last layer of A + 1 rows; "gauss": the Gaussian policy (policy.py:38-55) = head -> l -> (mu | log_std), raw, stacked into ONE last layer of 2A rows

    def __init__(self, state_size, action_size, num_support, hidden, head, max_batch, device, kind="rainbow", noise_type="factorized"):
        self._open(device)
        self.kind = kind
        self.cnn = head == "cnn"
        if self.cnn:
            self.Cin, self.Hin, self.Win = (int(v) for v in state_size)
        else:
            self.Cin, self.Hin, self.Win = int(state_size), 0, 0
        self.H, self.A, self.K, self.maxB = int(hidden), int(action_size), int(num_support), int(max_batch)
        if kind == "pv":
            self.n_actions, self.A = self.A, self.A + 1  # the library sees a q-network with one more output row: the value head
        if kind == "gauss":
            self.n_actions, self.A = self.A, 2 * self.A  # the Gaussian policy (policy.py:38-55) = a q-network with 2A output rows: mu | log_std, raw
        if kind in ("pv2", "gauss2"):
            # the policy-value nets with two value heads (policy_value.py:25-35, 60-70) = a q-network whose last layer stacks (pi | v | v_i) in
            # A + 2 rows or (mu | log_std | v | v_i), raw, in 2A + 2 rows
            self.n_actions, self.A = self.A, (self.A if kind == "pv2" else 2 * self.A) + 2
        kid = self._KIND[kind]
        self.noise_type = noise_type
        if kind in ("rainbow", "noisy") and noise_type == "independent":
            kid += 3 if kind == "rainbow" else 1
        n = int(self.lib.jh_rbnet_param_count_for(kid, int(self.cnn), self.Cin, self.Hin, self.Win, self.H, self.A, self.K))
        if n <= 0:
            L.check(-2)
        self.n_params = n
        self.params, self.target, self.grads, self.m, self.v = self._zeros(n)
        self.h = C.c_void_p()
        L.check(self.lib.jh_rbnet_create(self.ctx, kid, int(self.cnn), self.Cin, self.Hin, self.Win, self.H, self.A, self.K, self.maxB, L.ptr(self.params),
                                         L.ptr(self.target), L.ptr(self.grads), L.ptr(self.m), L.ptr(self.v), C.byref(self.h)))
        self.noise_len = int(self.lib.jh_rbnet_noise_len(self.h)) if kind in ("rainbow", "noisy") else 0
        self.seg = self._segments(self._SEG)
        if self.cnn:
            d1 = ((self.Hin - 8) // 4 + 1, (self.Win - 8) // 4 + 1)
            d2 = ((d1[0] - 4) // 2 + 1, (d1[1] - 4) // 2 + 1)
            self.d3 = (d2[0] - 2, d2[1] - 2)

    # ---- state_dict <-> private layout ---------------------------------------------------------
    def _v(self, bucket, name):
        off, rows, cols = self.seg[name]
        return bucket[off : off + rows * cols].view(rows, cols)

    def _feat_cols(self, w):
        """[R][F] weight that reads the head's features: the CNN head's features are (y, x, c) here and
        (c, y, x) in the reference -> a 4-D [R][c][y][x] view (export reshapes it, import views the source)."""
        return w.view(w.shape[0], self.d3[0], self.d3[1], 64).permute(0, 3, 1, 2) if self.cnn else w

    def _pairs(self, bucket):
        """[(reference key, view of the bucket shaped / strided like the reference tensor)] in the order of
        the reference module's state_dict (own parameters first, then sub-modules in registration order)."""
        H = self.H
        out, head = [], []
        if self.cnn:
            head.append(("head.conv1.weight", self._v(bucket, "w1").view(32, self.Cin, 8, 8)))
            head.append(("head.conv1.bias", self._v(bucket, "b1").view(-1)))
            head.append(("head.conv2.weight", self._v(bucket, "w2").view(64, 4, 4, 32).permute(0, 3, 1, 2)))
            head.append(("head.conv2.bias", self._v(bucket, "b2").view(-1)))
            head.append(("head.conv3.weight", self._v(bucket, "w3").view(64, 3, 3, 64).permute(0, 3, 1, 2)))
            head.append(("head.conv3.bias", self._v(bucket, "b3").view(-1)))
        else:
            head.append(("head.l.weight", self._v(bucket, "w1")))
            head.append(("head.l.bias", self._v(bucket, "b1").view(-1)))
        if self.kind == "rainbow":
            av1 = {k: self._v(bucket, f"{k}_av1") for k in ("mu", "sig")}
            bav1 = {k: self._v(bucket, f"{k}b_av1").view(-1) for k in ("mu", "sig")}
            for tag, sl in (("a1", slice(0, H)), ("v1", slice(H, 2 * H))):
                out += [(f"mu_w_{tag}", av1["mu"][sl].t()), (f"sig_w_{tag}", av1["sig"][sl].t()), (f"mu_b_{tag}", bav1["mu"][sl]), (f"sig_b_{tag}", bav1["sig"][sl])]
            for tag in ("a2", "v2"):
                out += [(f"mu_w_{tag}", self._v(bucket, f"mu_{tag}").t()), (f"sig_w_{tag}", self._v(bucket, f"sig_{tag}").t()),
                        (f"mu_b_{tag}", self._v(bucket, f"mub_{tag}").view(-1)), (f"sig_b_{tag}", self._v(bucket, f"sigb_{tag}").view(-1))]
            out += head
            out += [("l.weight", self._feat_cols(self._v(bucket, "wl"))), ("l.bias", self._v(bucket, "bl").view(-1))]
        elif self.kind == "noisy":  # network/noisy.py:15-20: mu_w1 / sig_w1 are [F][H] there (features (c, y, x)), [H][F] with (y, x, c) columns here
            for i, tag in ((1, "av1"), (2, "a2")):
                mu, sig = self._v(bucket, f"mu_{tag}"), self._v(bucket, f"sig_{tag}")
                if i == 1:
                    mu, sig = self._feat_cols(mu), self._feat_cols(sig)
                out += [(f"mu_w{i}", self._rows_last(mu)), (f"sig_w{i}", self._rows_last(sig)),
                        (f"mu_b{i}", self._v(bucket, f"mub_{tag}").view(-1)), (f"sig_b{i}", self._v(bucket, f"sigb_{tag}").view(-1))]
            out += head
        elif self.kind == "dueling":
            av1, bav1 = self._v(bucket, "mu_av1"), self._v(bucket, "mub_av1").view(-1)
            out += head
            out += [("l1_a.weight", self._feat_cols(av1[:H])), ("l1_a.bias", bav1[:H]), ("l1_v.weight", self._feat_cols(av1[H:])), ("l1_v.bias", bav1[H:]),
                    ("l2_a.weight", self._v(bucket, "mu_a2")), ("l2_a.bias", self._v(bucket, "mub_a2").view(-1)),
                    ("l2_v.weight", self._v(bucket, "mu_v2")), ("l2_v.bias", self._v(bucket, "mub_v2").view(-1))]
        elif self.kind == "pv":
            w, b, n = self._v(bucket, "mu_a2"), self._v(bucket, "mub_a2").view(-1), self.n_actions
            out += head
            out += [("l.weight", self._feat_cols(self._v(bucket, "wl"))), ("l.bias", self._v(bucket, "bl").view(-1)),
                    ("pi.weight", w[:n]), ("pi.bias", b[:n]), ("v.weight", w[n:]), ("v.bias", b[n:])]
        elif self.kind == "gauss":
            w, b, n = self._v(bucket, "mu_a2"), self._v(bucket, "mub_a2").view(-1), self.n_actions
            out += head
            out += [("l.weight", self._feat_cols(self._v(bucket, "wl"))), ("l.bias", self._v(bucket, "bl").view(-1)),
                    ("mu.weight", w[:n]), ("mu.bias", b[:n]), ("log_std.weight", w[n:]), ("log_std.bias", b[n:])]
        elif self.kind in ("pv2", "gauss2"):
            w, b, n = self._v(bucket, "mu_a2"), self._v(bucket, "mub_a2").view(-1), self.n_actions
            out += head
            out += [("l.weight", self._feat_cols(self._v(bucket, "wl"))), ("l.bias", self._v(bucket, "bl").view(-1))]
            names = ("pi",) if self.kind == "pv2" else ("mu", "log_std")
            for i, name in enumerate(names):
                out += [(f"{name}.weight", w[i * n : (i + 1) * n]), (f"{name}.bias", b[i * n : (i + 1) * n])]
            nv = len(names) * n
            out += [("v.weight", w[nv : nv + 1]), ("v.bias", b[nv : nv + 1]), ("v_i.weight", w[nv + 1 :]), ("v_i.bias", b[nv + 1 :])]
        else:
            last = "pi" if self.kind == "pi" else "q"  # "pi": the discrete policy (policy.py:23-35) = a q-network whose last layer is named pi
            out += head
            out += [("l.weight", self._feat_cols(self._v(bucket, "wl"))), ("l.bias", self._v(bucket, "bl").view(-1)),
                    (f"{last}.weight", self._v(bucket, "mu_a2")), (f"{last}.bias", self._v(bucket, "mub_a2").view(-1))]
        return out

    @staticmethod
    def _rows_last(w):
        """The reference's [in][out] view of a noisy weight kept [out][in] ([out][c][y][x] on the cnn head's features -> [c][y][x][out])."""
        return w.permute(*range(1, w.dim()), 0)

    @staticmethod
    def _is_feat_cols(k, v):
        return v.dim() == 4 and not k.startswith("head.")

    def export_state(self, bucket=None):
        bucket = self.params if bucket is None else bucket
        flat = (lambda v: v.reshape(-1, v.shape[-1])) if self.kind == "noisy" else (lambda v: v.reshape(v.shape[0], -1))
        return _export_pairs((k, flat(v) if self._is_feat_cols(k, v) else v) for k, v in self._pairs(bucket))

    def import_state(self, sd, bucket=None):
        bucket = self.params if bucket is None else bucket
        shape4 = (lambda v: (64, self.d3[0], self.d3[1], v.shape[-1])) if self.kind == "noisy" else (lambda v: (v.shape[0], 64, self.d3[0], self.d3[1]))
        _import_pairs(self._pairs(bucket), sd, self.device, lambda k, v, src: src.view(shape4(v)) if self._is_feat_cols(k, v) else src)

    # ---- engine ---------------------------------------------------------------------------------
    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0, centered=False):
        """Adam: (lr, beta1, beta2, eps); RMSprop: (lr, alpha -> beta1, -, eps, centered)."""
        L.check(self.lib.jh_rbnet_set_hyper(self.h, float(lr), float(beta1), float(beta2), float(eps), int(step), int(bool(centered)), L.stream_ptr()))

    def set_lr(self, lr):
        L.check(self.lib.jh_rbnet_set_lr(self.h, float(lr), L.stream_ptr()))

    def sync_target(self):
        L.check(self.lib.jh_rbnet_sync_target(self.h, L.stream_ptr()))

    def _xdt(self, x):
        if x.dtype == torch.uint8:
            return L.JH_U8
        if x.dtype == torch.float32:
            return L.JH_F32
        raise TypeError(f"observations must be uint8 or float32 on the device, got {x.dtype}")

    def forward(self, x, which=0, noise=None, out=None):
        """network(x, is_train = noise is not None) -> logits [rows, A, K]; rows <= max_batch."""
        assert x.is_contiguous() and x.device == self.device
        rows = int(x.shape[0])
        if out is None:
            out = torch.empty(rows, self.A, self.K, dtype=torch.float32, device=self.device)
        L.check(self.lib.jh_rbnet_forward(self.h, int(which), L.ptr(x), self._xdt(x), rows, L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def forward_keep(self, x, out):
        """network(x) of the online parameters with the activations kept for `backward` (an on-policy learner's forward: jh_rbnet_forward_keep)."""
        assert x.is_contiguous() and out.is_contiguous() and x.device == self.device
        L.check(self.lib.jh_rbnet_forward_keep(self.h, L.ptr(x), self._xdt(x), int(x.shape[0]), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward(self, x_all, B, noise, out):
        """x_all = [state; next_state] (2B rows), noise [3, noise_len] (rainbow; else None) -> out [3, B, A, K]."""
        assert x_all.is_contiguous() and (noise is None or noise.is_contiguous()) and out.is_contiguous() and int(x_all.shape[0]) == 2 * B
        L.check(self.lib.jh_rbnet_learn_forward(self.h, L.ptr(x_all), self._xdt(x_all), int(B), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def reserve_target_rows(self, rows):
        """Room for `rows` (<= 2 * max_batch) rows in the target network's activation buffers (jh_rbnet_reserve_target_rows): `learn_forward_m`
        needs 2B.  Allocates: call it once, outside any graph capture."""
        L.check(self.lib.jh_rbnet_reserve_target_rows(self.h, int(rows)))

    def learn_forward_m(self, x_all, B, noise, out):
        """x_all = [state; next_state] (2B rows) -> out [3, B, A, K] = online(state), target(state), target(next_state) (jh_rbnet_learn_forward_m);
        `backward` continues from it as after `learn_forward`.  q / dueling networks; `noise` is ignored."""
        assert x_all.is_contiguous() and out.is_contiguous() and int(x_all.shape[0]) == 2 * B
        L.check(self.lib.jh_rbnet_learn_forward_m(self.h, L.ptr(x_all), self._xdt(x_all), int(B), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward_p(self, x_all, B, noise, out):
        """x_all = [state; next_state] (2B rows) -> out [3, B, A, K] = online(state), online(next_state), target(state) (jh_rbnet_learn_forward_p):
        the forwards of MPO's discrete actor; `backward` continues from it as after `learn_forward`.  q / dueling networks; `noise` is ignored."""
        assert x_all.is_contiguous() and out.is_contiguous() and int(x_all.shape[0]) == 2 * B
        L.check(self.lib.jh_rbnet_learn_forward_p(self.h, L.ptr(x_all), self._xdt(x_all), int(B), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward_n(self, x_all, B, noise, out):
        """x_all = [state; next_state] (2B rows), noise [2, noise_len] -> out [2, B, A, 1] = online(state; noise 0), target(next_state; noise 1)
        (jh_rbnet_learn_forward_n: the two forwards of Noisy.learn, agent/noisy.py:83-105; the online trunk sees the first B rows only, the
        target trunk the last B); `backward` continues from it.  The noisy network only."""
        assert x_all.is_contiguous() and noise.is_contiguous() and out.is_contiguous() and int(x_all.shape[0]) == 2 * B
        assert noise.numel() >= 2 * self.noise_len and out.numel() >= 2 * B * self.A * self.K
        L.check(self.lib.jh_rbnet_learn_forward_n(self.h, L.ptr(x_all), self._xdt(x_all), int(B), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def sig_abs_mean(self, out=None):
        """Noisy.get_sig_w_mean (network/noisy.py:46-50) of the online parameters -> out f32[2] = {mean |sig_w1|, mean |sig_w2|}, one launch
        with a fixed summation order (jh_rbnet_sig_abs_mean).  The noisy network only."""
        if out is None:
            out = torch.empty(2, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= 2
        L.check(self.lib.jh_rbnet_sig_abs_mean(self.h, L.ptr(out), L.stream_ptr()))
        return out

    def hyper_ptr(self):
        """Device address of the optimizer's hyper block (jh_rbnet_hyper_ptr): what ops.mpo_loss_discrete takes as `hyper`."""
        return int(self.lib.jh_rbnet_hyper_ptr(self.h) or 0)

    def prepare_noise(self, noise):
        """The three noisy weight sets of learn()'s forwards for the draw `noise` [3, noise_len], on the CURRENT stream (may be a side stream)."""
        L.check(self.lib.jh_rbnet_prepare_noise(self.h, L.ptr(noise), L.stream_ptr()))

    def learn_trunk(self, x_all, B):
        assert x_all.is_contiguous() and int(x_all.shape[0]) == 2 * B
        L.check(self.lib.jh_rbnet_learn_trunk(self.h, L.ptr(x_all), self._xdt(x_all), int(B), L.stream_ptr()))

    def learn_heads(self, B, noise, out):
        assert (noise is None or noise.is_contiguous()) and out.is_contiguous()
        L.check(self.lib.jh_rbnet_learn_heads(self.h, int(B), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def learn_heads_raw(self, B, noise):
        """learn_heads up to the advantage / value streams; `c51_step` forms the logits inside the loss kernel."""
        assert noise is None or noise.is_contiguous()
        L.check(self.lib.jh_rbnet_learn_heads_raw(self.h, int(B), L.ptr(noise), L.stream_ptr()))

    def c51_step(self, tree, idx, action, reward, done, weights, v_min, v_max, gamma, alpha, n_step, logits, stats=None):
        """Rainbow.learn()'s loss step in three launches (jh_rbnet_c51_step): dueling combine of the three forwards (-> logits [3, B, A, K])
        + double-Q projection + KL + the gradient back through the combine (stays in the network: `backward(None)`); statistics + the
        priorities KL^alpha into the leaves `idx` (tree space, int64) of `tree` (ops.SumTree or None); the climb.  -> (prio [B], kl [B], stats f32[8])."""
        lib = self.lib
        B = int(logits.shape[1])
        assert logits.is_contiguous() and logits.dtype == torch.float32 and tuple(logits.shape) == (3, B, self.A, self.K)
        prio = torch.empty(B, dtype=torch.float32, device=self.device)
        kl = torch.empty(B, dtype=torch.float32, device=self.device)
        if stats is None:
            stats = torch.empty(8, dtype=torch.float32, device=self.device)
        r, d = _f32(reward).reshape(B, -1), _f32(done).reshape(B, -1)
        assert r.shape[1] == max(n_step, 1) and d.shape == r.shape
        flags = L.JH_C51_DOUBLE | (L.JH_C51_PER if weights is not None else 0)
        if tree is not None:
            assert idx.dtype == torch.int64 and idx.is_cuda and idx.is_contiguous() and idx.numel() == B
        L.check(lib.jh_rbnet_c51_step(self.h, None if tree is None else tree.h, B, int(n_step), flags, L.ptr(_f32(action).reshape(-1)), L.ptr(r), L.ptr(d),
                                      L.ptr(None if weights is None else _f32(weights).reshape(-1)), L.ptr(None if tree is None else idx), float(v_min), float(v_max),
                                      float(gamma), float(alpha), L.ptr(logits), L.ptr(prio), L.ptr(kl), L.ptr(stats), L.stream_ptr()))
        return prio, kl, stats

    def backward(self, g, defer=False):
        """g = d(loss)/d(logits of online(state)), or None after `c51_step`.  defer: leave d(sigma) = d(mu) * eps and the sum of conv1's
        weight-gradient partials to `optim_step` (it folds them into the optimizer pass when there is no clipping); `flush_grads`
        completes the bucket for a reader in between."""
        assert g is None or (g.is_contiguous() and g.dtype == torch.float32)
        fn = self.lib.jh_rbnet_backward_deferred if defer else self.lib.jh_rbnet_backward
        L.check(fn(self.h, L.ptr(g), L.stream_ptr()))

    def flush_grads(self):
        L.check(self.lib.jh_rbnet_flush_grads(self.h, L.stream_ptr()))

    def adam_step(self):
        L.check(self.lib.jh_rbnet_adam_step(self.h, L.stream_ptr()))

    def optim_step(self, optimizer="adam", max_norm=None):
        """[clip_grad_norm_(max_norm)] + optimizer.step(); optimizer in {"adam", "rmsprop"}."""
        L.check(self.lib.jh_rbnet_optim_step(self.h, {"adam": 0, "rmsprop": 1}[optimizer], float(max_norm or 0.0), L.stream_ptr()))


class IQNNet(_NetObject):
    """jh_iqnnet_*: the implicit quantile network with an MLP head (network/iqn.py:9-47) -- head.l, state_embed, cosine features of the
    caller's tau draws, sample_embed, Hadamard product, l1, l2, q -- with the three learn() forwards, the backward and Adam as tile-engine
    launches plus the elementwise kernels of jh_iqn.hip.  It presents RainbowNet's surface (flat buckets, export / import in the
    reference's state_dict keys, set_hyper / set_lr / sync_target, forward / learn_forward / backward / optim_step), so the agents'
    native plumbing (NativeValueNetMixin) works on it unchanged.  Outputs are [rows, N, A]; K = N.

    Where RainbowNet takes a noise draw, this takes tau: `forward(x, which, tau)` with tau [rows, N], `learn_forward(x_all, B, tau, out)`
    with tau [3, B, N].  forward() without tau draws it uniformly in `tau_range` on the device (torch.rand), or takes `tau_inject`."""

    _SEG = ("head.l.weight", "head.l.bias", "state_embed.weight", "state_embed.bias", "sample_embed.weight", "sample_embed.bias", "l1.weight", "l1.bias",
            "l2.weight", "l2.bias", "q.weight", "q.bias")
    _SYM = "jh_iqnnet_"
    kind, cnn, noise_len = "iqn", False, 0

    def __init__(self, state_size, action_size, embedding_dim, num_sample, hidden, max_batch, device):
        self._open(device)
        self.S, self.A, self.E, self.N, self.H, self.maxB = int(state_size), int(action_size), int(embedding_dim), int(num_sample), int(hidden), int(max_batch)
        self.K = self.N
        self.tau_range, self.tau_inject = (0.0, 1.0), None
        n = int(self._fn("param_count_for")(self.S, self.H, self.E, self.N, self.A))
        if n <= 0:
            L.check(-2)
        self.n_params = n
        self.params, self.target, self.grads, self.m, self.v = self._zeros(n)
        self.h = C.c_void_p()
        L.check(self._fn("create")(self.ctx, self.S, self.H, self.E, self.N, self.A, self.maxB, L.ptr(self.params), L.ptr(self.target), L.ptr(self.grads),
                                   L.ptr(self.m), L.ptr(self.v), C.byref(self.h)))
        assert int(self._fn("segment_count")()) == len(self._SEG)
        self.seg = self._segments(self._SEG)

    def _pairs(self, bucket):
        """[(reference key, view of the bucket shaped like the reference tensor)] in the order of the reference module's state_dict."""
        return _seg_pairs(bucket, self.seg)

    def export_state(self, bucket=None):
        return _export_pairs(self._pairs(self.params if bucket is None else bucket))

    def import_state(self, sd, bucket=None):
        _import_pairs(self._pairs(self.params if bucket is None else bucket), sd, self.device)

    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0, centered=False):
        L.check(self._fn("set_hyper")(self.h, float(lr), float(beta1), float(beta2), float(eps), int(step), L.stream_ptr()))

    def set_lr(self, lr):
        L.check(self._fn("set_lr")(self.h, float(lr), L.stream_ptr()))

    def sync_target(self):
        L.check(self._fn("sync_target")(self.h, L.stream_ptr()))

    def draw_tau(self, rows, lo=None, hi=None):
        """tau [rows, N] on the device: the injected draw, or uniform in [lo, hi] (default `tau_range`) like the reference's uniform_ (iqn.py:41-45)."""
        if self.tau_inject is not None:
            return torch.as_tensor(self.tau_inject).to(self.device, torch.float32).reshape(rows, self.N).contiguous()
        lo, hi = self.tau_range if lo is None else (lo, hi)
        t = torch.rand(rows, self.N, device=self.device)
        return t if (lo, hi) == (0.0, 1.0) else t * (hi - lo) + lo

    def forward(self, x, which=0, tau=None, out=None):
        """network(x) -> logits [rows, N, A]; rows <= max_batch.  tau [rows, N] or None (see draw_tau)."""
        assert x.is_contiguous() and x.device == self.device and x.dtype == torch.float32
        rows = int(x.shape[0])
        tau = self.draw_tau(rows) if tau is None else tau
        assert tau.is_contiguous() and tau.dtype == torch.float32 and tau.numel() == rows * self.N and tau.device == self.device
        if out is None:
            out = torch.empty(rows, self.N, self.A, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.numel() == rows * self.N * self.A
        L.check(self._fn("forward")(self.h, int(which), L.ptr(x), rows, L.ptr(tau), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward(self, x_all, B, tau, out):
        """x_all = [state; next_state] (2B rows), tau [3, B, N] -> out [3, B, N, A] = online(state), online(next_state), target(next_state)."""
        assert x_all.is_contiguous() and x_all.dtype == torch.float32 and int(x_all.shape[0]) == 2 * B
        assert tau.is_contiguous() and tau.dtype == torch.float32 and tau.numel() == 3 * B * self.N
        assert out.is_contiguous() and out.numel() == 3 * B * self.N * self.A
        L.check(self._fn("learn_forward")(self.h, L.ptr(x_all), int(B), L.ptr(tau), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward_m(self, x_all, B, tau, out):
        """M-IQN's arrangement: x_all = [state; next_state] (2B rows), tau [3, B, N] -> out [3, B, N, A] = online(state) with draw 0 (the
        one backward differentiates), online(state) with draw 1, target(next_state) with draw 2."""
        assert x_all.is_contiguous() and x_all.dtype == torch.float32 and int(x_all.shape[0]) == 2 * B
        assert tau.is_contiguous() and tau.dtype == torch.float32 and tau.numel() == 3 * B * self.N
        assert out.is_contiguous() and out.numel() == 3 * B * self.N * self.A
        L.check(self._fn("learn_forward_m")(self.h, L.ptr(x_all), int(B), L.ptr(tau), L.ptr(out), L.stream_ptr()))
        return out

    def backward(self, g, defer=False):
        """g = d(loss)/d(logits of online(state)) [B, N, A]."""
        assert g.is_contiguous() and g.dtype == torch.float32
        L.check(self._fn("backward")(self.h, L.ptr(g), L.stream_ptr()))

    def optim_step(self, optimizer="adam", max_norm=None):
        """[clip_grad_norm_(max_norm)] + Adam's step."""
        if optimizer != "adam":
            raise ValueError(f"IQNNet has Adam only (every config.iqn.* uses it), got {optimizer!r}")
        L.check(self._fn("optim_step")(self.h, float(max_norm or 0.0), L.stream_ptr()))


class RainbowIQNNet(IQNNet):
    """jh_riqnnet_* on jh_iqnnet's object: IQN's trunk at the caller's width, then Rainbow's noisy dueling tail with one support over the
    rows x N sampled rows (network/rainbow_iqn.py:9-113).  IQNNet's surface with a noise draw beside tau: `forward(x, which, tau, noise)`
    (noise None = is_train False: W = mu), `learn_forward(x_all, B, tau, noise, out)` with tau [3, B, N] and noise [3, noise_len].  One noise
    set is RainbowNet's with K = 1: [ei_a1 H][ej_a1 H][ei_v1 H][ej_v1 H][ei_a2 H][ej_a2 A][ei_v2 H][ej_v2 1] (factorized), or eps_w [in, out]
    then eps_b per layer a1, v1, a2, v2 (independent)."""

    _SEG = IQNNet._SEG + ("mu_av1", "sig_av1", "mub_av1", "sigb_av1", "mu_a2", "sig_a2", "mub_a2", "sigb_a2", "mu_v2", "sig_v2", "mub_v2", "sigb_v2")
    kind = "rainbow_iqn"

    def __init__(self, state_size, action_size, embedding_dim, num_sample, hidden, max_batch, device, noise_type="factorized"):
        self._open(device)
        self.S, self.A, self.E, self.N, self.H, self.maxB = int(state_size), int(action_size), int(embedding_dim), int(num_sample), int(hidden), int(max_batch)
        self.K = self.N
        self.noise_type = noise_type
        self.tau_range, self.tau_inject = (0.0, 1.0), None
        self.act_noise = None  # the draw of a forward() that is given none (the agent's act() in training mode sets it around its call)
        n = int(self.lib.jh_riqnnet_param_count_for(self.S, self.H, self.E, self.N, self.A))
        if n <= 0:
            L.check(-2)
        self.n_params = n
        self.params, self.target, self.grads, self.m, self.v = self._zeros(n)
        self.h = C.c_void_p()
        L.check(self.lib.jh_riqnnet_create(self.ctx, self.S, self.H, self.E, self.N, self.A, int(noise_type == "independent"), self.maxB, L.ptr(self.params),
                                           L.ptr(self.target), L.ptr(self.grads), L.ptr(self.m), L.ptr(self.v), C.byref(self.h)))
        assert int(self.lib.jh_riqnnet_segment_count()) == len(self._SEG)
        self.seg = self._segments(self._SEG)
        self.noise_len = int(self.lib.jh_riqnnet_noise_len(self.h))

    def _v(self, bucket, name):
        off, rows, cols = self.seg[name]
        return bucket[off : off + rows * cols].view(rows, cols)

    def _pairs(self, bucket):
        """The reference module's state_dict order: its own 16 noisy tensors (a1, v1, a2, v2: mu_w, sig_w, mu_b, sig_b, each weight [in, out]),
        then the submodules head.l, state_embed, sample_embed, l1, l2 (network/rainbow_iqn.py:13-38)."""
        H = self.H
        out = []
        av1 = {k: self._v(bucket, f"{k}_av1") for k in ("mu", "sig")}
        bav1 = {k: self._v(bucket, f"{k}b_av1").view(-1) for k in ("mu", "sig")}
        for tag, sl in (("a1", slice(0, H)), ("v1", slice(H, 2 * H))):
            out += [(f"mu_w_{tag}", av1["mu"][sl].t()), (f"sig_w_{tag}", av1["sig"][sl].t()), (f"mu_b_{tag}", bav1["mu"][sl]), (f"sig_b_{tag}", bav1["sig"][sl])]
        for tag in ("a2", "v2"):
            out += [(f"mu_w_{tag}", self._v(bucket, f"mu_{tag}").t()), (f"sig_w_{tag}", self._v(bucket, f"sig_{tag}").t()),
                    (f"mu_b_{tag}", self._v(bucket, f"mub_{tag}").view(-1)), (f"sig_b_{tag}", self._v(bucket, f"sigb_{tag}").view(-1))]
        trunk = {k: v for k, v in self.seg.items() if "." in k and not k.startswith("q.")}
        return out + _seg_pairs(bucket, trunk)

    def forward(self, x, which=0, tau=None, noise=None, out=None):
        """network(x, is_train = noise is not None) -> logits [rows, N, A]; rows <= max_batch.  tau [rows, N] or None (see draw_tau);
        noise None: `act_noise`, else W = mu."""
        assert x.is_contiguous() and x.device == self.device and x.dtype == torch.float32
        rows = int(x.shape[0])
        tau = self.draw_tau(rows) if tau is None else tau
        noise = self.act_noise if noise is None else noise
        assert tau.is_contiguous() and tau.dtype == torch.float32 and tau.numel() == rows * self.N and tau.device == self.device
        assert noise is None or (noise.is_contiguous() and noise.dtype == torch.float32 and noise.numel() == self.noise_len and noise.device == self.device)
        if out is None:
            out = torch.empty(rows, self.N, self.A, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.numel() == rows * self.N * self.A
        L.check(self.lib.jh_riqnnet_forward(self.h, int(which), L.ptr(x), rows, L.ptr(tau), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward(self, x_all, B, tau, noise, out):
        """x_all = [state; next_state] (2B rows), tau [3, B, N], noise [3, noise_len] -> out [3, B, N, A] = online(state), online(next_state),
        target(next_state), forward i under tau draw i and noise draw i."""
        assert x_all.is_contiguous() and x_all.dtype == torch.float32 and int(x_all.shape[0]) == 2 * B
        assert tau.is_contiguous() and tau.dtype == torch.float32 and tau.numel() == 3 * B * self.N
        assert noise.is_contiguous() and noise.dtype == torch.float32 and noise.numel() == 3 * self.noise_len
        assert out.is_contiguous() and out.numel() == 3 * B * self.N * self.A
        L.check(self.lib.jh_riqnnet_learn_forward(self.h, L.ptr(x_all), int(B), L.ptr(tau), L.ptr(noise), L.ptr(out), L.stream_ptr()))
        return out

    def learn_forward_m(self, *a, **k):
        raise NotImplementedError("RainbowIQNNet has Rainbow-IQN's arrangement of forwards only")


class R2D2Net(_NetObject):
    """jh_r2d2net_*: R2D2's recurrent dueling network (core/network/r2d2.py) with an MLP head -- the three sequence passes of learn() in
    lockstep (one LSTM step launch per time step for all three), backpropagation through time over the trained steps, clip + Adam over the
    flat bucket, and the one-step acting forward.  Buckets, export / import under the reference's 16 state_dict keys, set_hyper / set_lr /
    sync_target / optim_step as the other network objects have them."""

    # the library's segment order (l1_a | l1_v and their biases sit next to each other); state_dict order is the reference's
    _SEG = ("head.l.weight", "head.l.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "l.weight", "l.bias",
            "l1_a.weight", "l1_v.weight", "l1_a.bias", "l1_v.bias", "l2_a.weight", "l2_a.bias", "l2_v.weight", "l2_v.bias")
    _KEYS = ("head.l.weight", "head.l.bias", "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "l.weight", "l.bias",
             "l1_a.weight", "l1_a.bias", "l1_v.weight", "l1_v.bias", "l2_a.weight", "l2_a.bias", "l2_v.weight", "l2_v.bias")
    _SYM = "jh_r2d2net_"
    kind, cnn, noise_len = "r2d2", False, 0

    def __init__(self, state_size, action_size, hidden, max_batch, seq_len, n_burn_in, n_step, device):
        self._open(device)
        self.S, self.A, self.H, self.maxB = int(state_size), int(action_size), int(hidden), int(max_batch)
        self.seq_len, self.n_burn_in, self.n_step = int(seq_len), int(n_burn_in), int(n_step)
        n = int(self._fn("param_count_for")(self.S, self.H, self.A))
        if n <= 0:
            L.check(-2)
        self.n_params = n
        self.params, self.target, self.grads, self.m, self.v = self._zeros(n)
        self.h = C.c_void_p()
        L.check(self._fn("create")(self.ctx, self.S, self.H, self.A, self.maxB, self.seq_len, self.n_burn_in, self.n_step, L.ptr(self.params), L.ptr(self.target),
                                   L.ptr(self.grads), L.ptr(self.m), L.ptr(self.v), C.byref(self.h)))
        assert int(self._fn("segment_count")()) == len(self._SEG)
        self.seg = self._segments(self._SEG)

    def _pairs(self, bucket):
        """[(reference key, view of the bucket shaped like the reference tensor)] in the order of the reference module's state_dict."""
        out = []
        for k in self._KEYS:
            off, rows, cols = self.seg[k]
            v = bucket[off : off + rows * cols]
            out.append((k, v.view(rows, cols) if ".weight" in k else v))  # (lstm.weight_ih_l0 does not END in .weight)
        return out

    def export_state(self, bucket=None):
        return _export_pairs(self._pairs(self.params if bucket is None else bucket))

    def import_state(self, sd, bucket=None):
        _import_pairs(self._pairs(self.params if bucket is None else bucket), sd, self.device)

    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0, centered=False):
        L.check(self._fn("set_hyper")(self.h, float(lr), float(beta1), float(beta2), float(eps), int(step), L.stream_ptr()))

    def set_lr(self, lr):
        L.check(self._fn("set_lr")(self.h, float(lr), L.stream_ptr()))

    def sync_target(self):
        L.check(self._fn("sync_target")(self.h, L.stream_ptr()))

    def learn_forward(self, state, onehot, hidden_h, hidden_c, next_hidden_h, next_hidden_c, out=None):
        """state [B, seq_len + n_step, S], onehot [B, seq_len + n_step, A], the four stored states [B, H] (or [B, 1, H])
        -> out [3, seq_len - n_burn_in, B, A] time-major = online over state[:, :seq_len], online and target over state[:, n_step:]."""
        t = [_f32(v) for v in (state, onehot, hidden_h, hidden_c, next_hidden_h, next_hidden_c)]
        B, Ls = int(t[0].shape[0]), self.seq_len + self.n_step
        assert tuple(t[0].shape) == (B, Ls, self.S) and tuple(t[1].shape) == (B, Ls, self.A) and all(v.numel() == B * self.H for v in t[2:])
        Tt = self.seq_len - self.n_burn_in
        if out is None:
            out = torch.empty(3, Tt, B, self.A, dtype=torch.float32, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() == 3 * Tt * B * self.A
        L.check(self._fn("learn_forward")(self.h, *(L.ptr(v) for v in t), B, L.ptr(out), L.stream_ptr()))
        return out

    def backward(self, g, defer=False):
        """g = d(loss)/d(out[0]) [seq_len - n_burn_in, B, A]."""
        assert g.is_contiguous() and g.dtype == torch.float32
        L.check(self._fn("backward")(self.h, L.ptr(g), L.stream_ptr()))

    def optim_step(self, optimizer="adam", max_norm=None):
        """[clip_grad_norm_(max_norm)] + Adam's step."""
        if optimizer != "adam":
            raise ValueError(f"R2D2Net has Adam only (every config.r2d2.* uses it), got {optimizer!r}")
        L.check(self._fn("optim_step")(self.h, float(max_norm or 0.0), L.stream_ptr()))

    def act_step(self, x, prev_onehot, h, c, out=None):
        """One time step of the online network: x [N, S], prev_onehot [N, A], carried state h / c [N, H] -> (q [N, A], h', c'); out = the
        three tensors to write into."""
        x, p, h, c = _f32(x), _f32(prev_onehot), _f32(h), _f32(c)
        N = int(x.shape[0])
        assert tuple(x.shape) == (N, self.S) and tuple(p.shape) == (N, self.A) and tuple(h.shape) == (N, self.H) and tuple(c.shape) == (N, self.H)
        q, h1, c1 = out if out is not None else (torch.empty(N, self.A, dtype=torch.float32, device=self.device), torch.empty_like(h), torch.empty_like(c))
        L.check(self._fn("act_step")(self.h, L.ptr(x), L.ptr(p), L.ptr(h), L.ptr(c), N, L.ptr(q), L.ptr(h1), L.ptr(c1), L.stream_ptr()))
        return q, h1, c1


def td3_next_action(z, eps=None, noise_std=0.0, noise_clip=0.0, out=None):
    """jh_td3_next_action: clamp(tanh(z) + clamp(noise_std * eps, -noise_clip, noise_clip), -1, 1) on [B, A] (td3.py:159-162); eps None: tanh(z)."""
    z = _f32(z)
    B, A = z.shape
    eps = None if eps is None else _f32(eps)
    assert eps is None or tuple(eps.shape) == (B, A)
    out = torch.empty_like(z) if out is None else out
    L.check(L.load().jh_td3_next_action(L.ctx(z.device.index), B, A, L.ptr(z), L.ptr(eps), float(noise_std), float(noise_clip), L.ptr(out), L.stream_ptr()))
    return out


def td3_critic_loss(q, q_next, reward, done, gamma, stats=None):
    """jh_td3_critic_loss: q, q_next [n, B] (n = 1 or 2 critics) -> (y [B], d(loss_i)/d(q_i) [n, B], stats [4] = loss_1, loss_2, max_Q, mark)."""
    q, q_next, reward, done = _f32(q), _f32(q_next), _f32(reward), _f32(done)
    n, B = q.shape
    assert tuple(q_next.shape) == (n, B) and reward.numel() == B and done.numel() == B
    y = torch.empty(B, dtype=torch.float32, device=q.device)
    grad = torch.empty(n, B, dtype=torch.float32, device=q.device)
    stats = torch.zeros(4, dtype=torch.float32, device=q.device) if stats is None else stats
    L.check(L.load().jh_td3_critic_loss(L.ctx(q.device.index), B, n, L.ptr(q), L.ptr(q_next), L.ptr(reward), L.ptr(done), float(gamma), L.ptr(y), L.ptr(grad),
                                        L.ptr(stats), L.stream_ptr()))
    return y, grad, stats


def td3_actor_seed(q, stats=None):
    """jh_td3_actor_seed: q [B] -> (d(actor_loss)/d(q) [B] = -1 / B, stats [2] = actor_loss = -mean(q), mark)."""
    q = _f32(q).reshape(-1)
    B = q.numel()
    grad = torch.empty(B, dtype=torch.float32, device=q.device)
    stats = torch.zeros(2, dtype=torch.float32, device=q.device) if stats is None else stats
    L.check(L.load().jh_td3_actor_seed(L.ctx(q.device.index), B, L.ptr(q), L.ptr(grad), L.ptr(stats), L.stream_ptr()))
    return grad, stats


def td3_tanh_backward(grad_a, a):
    """jh_td3_tanh_backward: d(z) = d(a) * (1 - a^2) on [B, A]."""
    grad_a, a = _f32(grad_a), _f32(a)
    B, A = a.shape
    out = torch.empty_like(a)
    L.check(L.load().jh_td3_tanh_backward(L.ctx(a.device.index), B, A, L.ptr(grad_a), L.ptr(a), L.ptr(out), L.stream_ptr()))
    return out


def td3_polyak(params, target, tau):
    """jh_td3_polyak: target <- tau * params + (1 - tau) * target in place over flat float32 buckets (td3.py:203-209)."""
    assert params.is_contiguous() and target.is_contiguous() and params.dtype == target.dtype == torch.float32 and params.numel() == target.numel()
    L.check(L.load().jh_td3_polyak(L.ctx(params.device.index), int(params.numel()), L.ptr(params), L.ptr(target), float(tau), L.stream_ptr()))
    return target


class _ActorCriticBuckets(_NetObject):
    """What ACNet and SACNet share: an actor and `nc` critics in flat float32 buckets (`self.actor[kind]` of n_actor floats,
    `self.critics[kind]` of nc * n_critic floats, critic c at c * n_critic), the segment tables `aseg` / `cseg` name -> (offset, rows, cols),
    export / import under the reference's state_dict keys, and every native entry the two objects have in common, called as `_SYM + name`.
    Networks are named "actor", "critic1", "critic2" ("critic" = "critic1").  A subclass names its entries' prefix `_SYM`, the actor's
    segments `_ASEG` and buckets `AKINDS`, and the sizes its create entry takes."""

    _CSEG = ("head.l.weight", "head.l.bias", "e.weight", "e.bias", "l.weight", "l.bias", "q.weight", "q.bias")
    KINDS = AKINDS = ("params", "target", "grads", "m", "v")
    cnn = False

    def __init__(self, state_size, action_size, hidden, n_critics, max_batch, device):
        self._open(device)
        self.S, self.A, self.H, self.nc, self.maxB = int(state_size), int(action_size), int(hidden), int(n_critics), int(max_batch)
        na, ncr = C.c_int64(), C.c_int64()
        L.check(self._fn("param_counts_for")(self.S, self.H, self.A, C.byref(na), C.byref(ncr)))
        self.n_actor, self.n_critic = int(na.value), int(ncr.value)
        self.actor = dict(zip(self.AKINDS, self._zeros(self.n_actor, len(self.AKINDS))))
        self.critics = dict(zip(self.KINDS, self._zeros(self.nc * self.n_critic)))
        self.h = C.c_void_p()
        L.check(self._fn("create")(self.ctx, *self._create_sizes(), *[L.ptr(self.actor[k]) for k in self.AKINDS], *[L.ptr(self.critics[k]) for k in self.KINDS],
                                   C.byref(self.h)))
        assert int(self._fn("segment_count")()) == len(self._ASEG + self._CSEG)
        self.aseg, self.cseg = self._segments(self._ASEG), self._segments(self._CSEG, len(self._ASEG))

    def set_hyper(self, which, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0):
        """which: "actor" | "critic" (one Adam for both critics)."""
        L.check(self._fn("set_hyper")(self.h, 0 if which == "actor" else 1, float(lr), float(beta1), float(beta2), float(eps), int(step), L.stream_ptr()))

    def set_lr(self, which, lr):
        L.check(self._fn("set_lr")(self.h, 0 if which == "actor" else 1, float(lr), L.stream_ptr()))

    def sync_target(self):
        L.check(self._fn("sync_target")(self.h, L.stream_ptr()))

    def soft_update(self, tau):
        L.check(self._fn("soft_update")(self.h, float(tau), L.stream_ptr()))

    def critic_forward(self, x, action, which=0):
        """critic_c(x, action) for every critic -> [n_critics, rows]."""
        assert x.is_contiguous() and x.dtype == torch.float32 and action.is_contiguous() and action.dtype == torch.float32
        rows = int(x.shape[0])
        assert tuple(x.shape) == (rows, self.S) and tuple(action.shape) == (rows, self.A)
        out = torch.empty(self.nc, rows, dtype=torch.float32, device=self.device)
        L.check(self._fn("critic_forward")(self.h, int(which), L.ptr(x), L.ptr(action), rows, L.ptr(out), L.stream_ptr()))
        return out

    def _check_batch(self, x_all, action, reward, done, y, q):
        """The critic update's inputs x_all = [state; next_state] (2B rows), action [B, A], reward, done [B] and optional outputs -> B."""
        B = int(action.shape[0])
        for t in (x_all, action, reward, done):
            assert t.is_contiguous() and t.dtype == torch.float32
        assert tuple(x_all.shape) == (2 * B, self.S) and tuple(action.shape) == (B, self.A) and reward.numel() == B and done.numel() == B
        assert (y is None or y.numel() == B) and (q is None or q.numel() == self.nc * B)
        return B

    def nets(self):
        return ("actor",) + tuple(f"critic{c + 1}" for c in range(self.nc))

    def flat(self, net, kind="params"):
        """The flat float32 view of one network in one of the buckets KINDS."""
        if net == "actor":
            return self.actor[kind]
        c = {"critic": 0, "critic1": 0, "critic2": 1}[net]
        assert c < self.nc, f"{net}: this object has {self.nc} critic(s)"
        return self.critics[kind][c * self.n_critic : (c + 1) * self.n_critic]

    def _pairs(self, net, kind):
        return _seg_pairs(self.flat(net, kind), self.aseg if net == "actor" else self.cseg)

    def export_state(self, net, kind="params"):
        return _export_pairs(self._pairs(net, kind))

    def import_state(self, sd, net, kind="params"):
        _import_pairs(self._pairs(net, kind), sd, self.device)


class ACNet(_ActorCriticBuckets):
    """jh_acnet_*: a deterministic policy (network/policy.py:8-20) and one (DDPG) or two (TD3) continuous Q networks
    (network/q_network.py:23-39), each with a target copy, in flat buckets: `actor*` of n_actor floats, `critics*` of n_critics * n_critic
    floats (critic c at c * n_critic).  The critic update, the actor update (backward through critic 1's action input), the soft update
    and the target sync are tile-engine launches plus the elementwise kernels of jh_td3.hip and jh_acnet.hip.  Networks are named "actor", "critic1",
    "critic2" ("critic" = "critic1"); export / import speak the reference's state_dict keys."""

    _ASEG = ("head.l.weight", "head.l.bias", "l.weight", "l.bias", "pi.weight", "pi.bias")
    _SYM = "jh_acnet_"
    kind = "actor_critic"

    def _create_sizes(self):
        return self.S, self.H, self.A, self.nc, self.maxB

    def actor_forward(self, x, which=0, out=None):
        """actor(x) -> [rows, A]; rows <= max_batch; which 0 online / 1 target."""
        assert x.is_contiguous() and x.device == self.device and x.dtype == torch.float32 and x.shape[1] == self.S
        rows = int(x.shape[0])
        out = torch.empty(rows, self.A, dtype=torch.float32, device=self.device) if out is None else out
        assert out.is_contiguous() and out.numel() == rows * self.A
        L.check(self.lib.jh_acnet_actor_forward(self.h, int(which), L.ptr(x), rows, L.ptr(out), L.stream_ptr()))
        return out

    def critic_update(self, x_all, action, reward, done, noise, gamma, noise_std, noise_clip, stats, y=None, q=None):
        """x_all = [state; next_state] (2B rows); noise [B, A] standard normals or None.  stats [4] = loss_1, loss_2, max_Q, mark;
        optional outputs y [B], q [n_critics, B]."""
        B = self._check_batch(x_all, action, reward, done, y, q)
        assert noise is None or (noise.is_contiguous() and noise.dtype == torch.float32 and tuple(noise.shape) == (B, self.A))
        L.check(self.lib.jh_acnet_critic_update(self.h, L.ptr(x_all), L.ptr(action), L.ptr(reward), L.ptr(done), L.ptr(noise), B, float(gamma), float(noise_std),
                                                float(noise_clip), L.ptr(y), L.ptr(q), L.ptr(stats), L.stream_ptr()))

    def actor_update(self, x, stats, action_pred=None):
        """x = state [B, S]; stats [2] = actor_loss, mark; optional output action_pred [B, A] = actor(state) before the step."""
        B = int(x.shape[0])
        assert x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.S and (action_pred is None or action_pred.numel() == B * self.A)
        L.check(self.lib.jh_acnet_actor_update(self.h, L.ptr(x), B, L.ptr(action_pred), L.ptr(stats), L.stream_ptr()))

    # ---- critic 0 over sampled actions (continuous MPO)
    def reserve_sampled(self, rows):
        """Room for rows = N * R sampled rows (two slots); allocates: once, outside any capture."""
        L.check(self.lib.jh_acnet_reserve_sampled(self.h, int(rows)))

    def critic_forward_sampled(self, x, actions, which=0, out=None):
        """critic 0 of x [R, S] over actions [N, R, A] -> [N, R]; head.l(s) runs once per state row."""
        N, R, A = (int(v) for v in actions.shape)
        for t in (x, actions):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device
        assert tuple(x.shape) == (R, self.S) and A == self.A
        out = torch.empty(N, R, dtype=torch.float32, device=self.device) if out is None else out
        assert out.is_contiguous() and out.numel() == N * R and out.dtype == torch.float32
        L.check(self.lib.jh_acnet_critic_forward_sampled(self.h, int(which), L.ptr(x), L.ptr(actions), R, N, L.ptr(out), L.stream_ptr()))
        return out

    def mpo_forward(self, x_all, action, a_next, a_add, out=None):
        """x_all = [state; next_state] (2R rows), action [R, A], a_next / a_add [N, R, A].  out = (q [R], qt_a [R], qt_next [N, R], qt_add [N, R])
        to write into -> the four: online(s, a), target(s, a), target(s', a_next), target(s, a_add)."""
        N, R, A = (int(v) for v in a_next.shape)
        for t in (x_all, action, a_next, a_add):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device
        assert tuple(x_all.shape) == (2 * R, self.S) and action.numel() == R * self.A and A == self.A and tuple(a_add.shape) == (N, R, A)
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
        q, qt_a, qt_next, qt_add = out if out is not None else (f(R), f(R), f(N, R), f(N, R))
        assert all(t.is_contiguous() and t.dtype == torch.float32 for t in (q, qt_a, qt_next, qt_add))
        assert q.numel() == qt_a.numel() == R and qt_next.numel() == qt_add.numel() == N * R
        L.check(self.lib.jh_acnet_mpo_forward(self.h, L.ptr(x_all), L.ptr(action), L.ptr(a_next), L.ptr(a_add), R, N, L.ptr(q), L.ptr(qt_a), L.ptr(qt_next),
                                              L.ptr(qt_add), L.stream_ptr()))
        return q, qt_a, qt_next, qt_add

    def critic_fit(self, x, action, dq, max_norm=0.0):
        """The critic's backward from dq [R] (of the online q the last mpo_forward produced), clip_grad_norm_(max_norm) and its Adam step."""
        R = int(dq.numel())
        for t in (x, action, dq):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device
        assert tuple(x.shape) == (R, self.S) and action.numel() == R * self.A
        L.check(self.lib.jh_acnet_critic_fit(self.h, L.ptr(x), L.ptr(action), L.ptr(dq), R, float(max_norm or 0.0), L.stream_ptr()))


SAC_ALPHA_FLOATS = 16


def sac_alpha_block(log_alpha, alpha=None, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=0, m=0.0, v=0.0, dynamic=True, target_entropy=-1.0, device="cuda"):
    """The temperature's device block of the jh_sac_* kernels (include/jorldy_hip.h): log_alpha, the alpha in use (None: exp(log_alpha) rounded
    to float32), Adam's moments, step count and settings, the dynamic flag and target_entropy.  -> float32 [16] on `device`."""
    import math

    import numpy as np

    h = np.zeros(SAC_ALPHA_FLOATS, np.float32)
    la = np.float32(log_alpha)
    h[:9] = [la, math.exp(float(la)) if alpha is None else alpha, m, v, step, lr, eps, 1.0 if dynamic else 0.0, target_entropy]
    h[10:14] = np.asarray([beta1, beta2], np.float64).view(np.float32)
    return torch.from_numpy(h).to(device)


def sac_alpha_read(block):
    """-> dict(log_alpha, alpha, m, v, step, lr, eps, dynamic, target_entropy, coef) of a temperature block, as Python numbers."""
    h = block.detach().cpu().numpy()
    names = ("log_alpha", "alpha", "m", "v", "step", "lr", "eps", "dynamic", "target_entropy", "coef")
    out = {k: float(h[i]) for i, k in enumerate(names)}
    out["step"], out["dynamic"] = int(out["step"]), bool(out["dynamic"])
    return out


def sac_sample(mu_raw, ls_raw=None, eps=None, a=None, logp=None):
    """jh_sac_sample on [B, A] (sac.py:161-169, policy.py:38-55) -> (a [B, A], logp [B]); eps None: (tanh(clamp(mu_raw, -5, 5)), None)."""
    mu_raw = _f32(mu_raw)
    B, A = mu_raw.shape
    ls_raw = None if ls_raw is None else _f32(ls_raw)
    eps = None if eps is None else _f32(eps)
    assert eps is None or (ls_raw is not None and tuple(eps.shape) == (B, A) and tuple(ls_raw.shape) == (B, A))
    a = torch.empty_like(mu_raw) if a is None else a
    if eps is not None and logp is None:
        logp = torch.empty(B, dtype=torch.float32, device=mu_raw.device)
    assert a.numel() == B * A and (eps is None or logp.numel() == B)
    L.check(L.load().jh_sac_sample(L.ctx(mu_raw.device.index), B, A, L.ptr(mu_raw), L.ptr(ls_raw), L.ptr(eps), L.ptr(a), L.ptr(logp if eps is not None else None),
                                   L.stream_ptr()))
    return a, (logp if eps is not None else None)


def sac_critic_loss(q, q_next, logp_next, reward, done, gamma, alpha_block, stats=None):
    """jh_sac_critic_loss: q, q_next [2, B], logp_next [B] -> (y [B], d(loss_i)/d(q_i) [2, B], stats [4] = loss_1, loss_2, max_Q, mark)."""
    q, q_next, logp_next, reward, done = _f32(q), _f32(q_next), _f32(logp_next), _f32(reward), _f32(done)
    n, B = q.shape
    assert n == 2 and tuple(q_next.shape) == (2, B) and logp_next.numel() == B and reward.numel() == B and done.numel() == B
    assert alpha_block.dtype == torch.float32 and alpha_block.numel() == SAC_ALPHA_FLOATS and alpha_block.is_contiguous()
    y = torch.empty(B, dtype=torch.float32, device=q.device)
    grad = torch.empty(2, B, dtype=torch.float32, device=q.device)
    stats = torch.zeros(4, dtype=torch.float32, device=q.device) if stats is None else stats
    L.check(L.load().jh_sac_critic_loss(L.ctx(q.device.index), B, L.ptr(q), L.ptr(q_next), L.ptr(logp_next), L.ptr(reward), L.ptr(done), float(gamma),
                                        L.ptr(alpha_block), L.ptr(y), L.ptr(grad), L.ptr(stats), L.stream_ptr()))
    return y, grad, stats


def sac_actor_seed(q, logp, alpha_block, stats=None):
    """jh_sac_actor_seed: q [2, B], logp [B] -> (d(actor_loss)/d(q_i) [2, B], stats [6] = actor_loss, alpha_loss, mean_Q, alpha, entropy,
    mark).  Advances `alpha_block` in place: the coefficient alpha / B, and, dynamic, the alpha in use and one Adam step of log_alpha."""
    q, logp = _f32(q), _f32(logp).reshape(-1)
    n, B = q.shape
    assert n == 2 and logp.numel() == B
    assert alpha_block.dtype == torch.float32 and alpha_block.numel() == SAC_ALPHA_FLOATS and alpha_block.is_contiguous()
    grad = torch.empty(2, B, dtype=torch.float32, device=q.device)
    stats = torch.zeros(6, dtype=torch.float32, device=q.device) if stats is None else stats
    L.check(L.load().jh_sac_actor_seed(L.ctx(q.device.index), B, L.ptr(q), L.ptr(logp), L.ptr(alpha_block), L.ptr(grad), L.ptr(stats), L.stream_ptr()))
    return grad, stats


def sac_sample_backward(grad_a, mu_raw, ls_raw, eps, a, alpha_block, grad_a2=None):
    """jh_sac_sample_backward on [B, A]: d(a) (+ grad_a2) and the block's coefficient alpha / B -> (d(mu_raw), d(ls_raw))."""
    grad_a, mu_raw, ls_raw, eps, a = _f32(grad_a), _f32(mu_raw), _f32(ls_raw), _f32(eps), _f32(a)
    grad_a2 = None if grad_a2 is None else _f32(grad_a2)
    B, A = a.shape
    for t in (grad_a, mu_raw, ls_raw, eps) + (() if grad_a2 is None else (grad_a2,)):
        assert tuple(t.shape) == (B, A)
    assert alpha_block.dtype == torch.float32 and alpha_block.numel() == SAC_ALPHA_FLOATS and alpha_block.is_contiguous()
    dmu, dls = torch.empty_like(a), torch.empty_like(a)
    L.check(L.load().jh_sac_sample_backward(L.ctx(a.device.index), B, A, L.ptr(grad_a), L.ptr(grad_a2), L.ptr(mu_raw), L.ptr(ls_raw), L.ptr(eps), L.ptr(a),
                                            L.ptr(alpha_block), L.ptr(dmu), L.ptr(dls), L.stream_ptr()))
    return dmu, dls


class SACNet(_ActorCriticBuckets):
    """jh_sacnet_*: a Gaussian policy (network/policy.py:38-55), online only, and two continuous Q networks (network/q_network.py:23-39) with
    their targets, in the flat buckets of _ActorCriticBuckets (the actor has no "target" bucket), plus the temperature block of the jh_sac_* kernels.
    Networks are named "actor", "critic1", "critic2"; export / import speak the reference's state_dict keys."""

    _ASEG = ("head.l.weight", "head.l.bias", "l.weight", "l.bias", "mu.weight", "mu.bias", "log_std.weight", "log_std.bias")
    AKINDS = ("params", "grads", "m", "v")
    _SYM = "jh_sacnet_"
    kind = "soft_actor_critic"

    def __init__(self, state_size, action_size, hidden, max_batch, device):
        super().__init__(state_size, action_size, hidden, 2, max_batch, device)

    def _create_sizes(self):
        return self.S, self.H, self.A, self.maxB

    def set_alpha(self, log_alpha, alpha=None, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=0, m=0.0, v=0.0, dynamic=True):
        """The whole temperature block; alpha None: exp(log_alpha as float32).  Synchronises."""
        import math

        import numpy as np

        alpha = math.exp(float(np.float32(log_alpha))) if alpha is None else alpha
        L.check(self.lib.jh_sacnet_set_alpha(self.h, float(log_alpha), float(alpha), float(lr), float(beta1), float(beta2), float(eps), int(step), float(m), float(v),
                                             int(bool(dynamic)), L.stream_ptr()))

    def get_alpha(self):
        """-> dict(log_alpha, alpha, m, v, step, lr, eps, dynamic, target_entropy, coef, beta1, beta2).  Synchronises."""
        import numpy as np

        h = np.zeros(SAC_ALPHA_FLOATS, np.float32)
        L.check(self.lib.jh_sacnet_get_alpha(self.h, L.ptr(h), L.stream_ptr()))
        out = sac_alpha_read(torch.from_numpy(h))
        out["beta1"], out["beta2"] = (float(b) for b in h[10:14].view(np.float64))
        return out

    def actor_forward(self, x, which=0):
        """actor(x) -> (mu, std), each [rows, A]; rows <= max_batch.  There is no target actor."""
        assert which == 0 and x.is_contiguous() and x.device == self.device and x.dtype == torch.float32 and x.shape[1] == self.S
        rows = int(x.shape[0])
        mu, std = (torch.empty(rows, self.A, dtype=torch.float32, device=self.device) for _ in range(2))
        L.check(self.lib.jh_sacnet_actor_forward(self.h, L.ptr(x), rows, L.ptr(mu), L.ptr(std), L.stream_ptr()))
        return mu, std

    def critic_update(self, x_all, action, reward, done, eps, gamma, stats, y=None, q=None, a_next=None, logp_next=None):
        """x_all = [state; next_state] (2B rows); eps [B, A] standard normals.  stats [4] = loss_1, loss_2, max_Q, mark; optional outputs
        y [B], q [2, B], a_next [B, A], logp_next [B]."""
        B = self._check_batch(x_all, action, reward, done, y, q)
        assert eps.is_contiguous() and eps.dtype == torch.float32 and tuple(eps.shape) == (B, self.A) and stats.numel() >= 4
        assert (a_next is None or a_next.numel() == B * self.A) and (logp_next is None or logp_next.numel() == B)
        L.check(self.lib.jh_sacnet_critic_update(self.h, L.ptr(x_all), L.ptr(action), L.ptr(reward), L.ptr(done), L.ptr(eps), B, float(gamma), L.ptr(y), L.ptr(q),
                                                 L.ptr(a_next), L.ptr(logp_next), L.ptr(stats), L.stream_ptr()))

    def actor_update(self, x, eps, stats, action=None, logp=None, q=None):
        """x = state [B, S], eps [B, A]; stats [6] = actor_loss, alpha_loss, mean_Q, alpha, entropy, mark; optional outputs action [B, A],
        logp [B], q [2, B] = q_i(state, action) with the critics as they stand."""
        B = int(x.shape[0])
        assert x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.S and eps.is_contiguous() and tuple(eps.shape) == (B, self.A)
        assert stats.numel() >= 6 and (action is None or action.numel() == B * self.A) and (logp is None or logp.numel() == B) and (q is None or q.numel() == 2 * B)
        L.check(self.lib.jh_sacnet_actor_update(self.h, L.ptr(x), L.ptr(eps), B, L.ptr(action), L.ptr(logp), L.ptr(q), L.ptr(stats), L.stream_ptr()))


class ICMNet(_NetObject):
    """jh_icmnet_*: ICM-PPO's curiosity module (network/icm.py:153-218) -- the feature trunk with batch norm under batch statistics and ELU,
    the forward and the inverse model, the running moments of observations and intrinsic reward, the reward filter -- with the no-grad reward
    pass over a rollout (`obs_update`, `reward`) and one minibatch update (`update`: forward, both losses, backward, clip, Adam) as tile-engine
    launches plus the kernels of jh_icm.hip.  The trainable tensors live in flat buckets in the reference's registration order (`_SEG`);
    everything that is a buffer-like Parameter in the reference (rms_obs, rms_ri, rff, the batch norms' running statistics) lives in the
    device statistics block (`stats()` / `set_stats()`, the reference's state_dict keys)."""

    _SEG = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "forward_fc1.weight", "forward_fc1.bias", "forward_fc2.weight", "forward_fc2.bias",
            "inverse_fc1.weight", "inverse_fc1.bias", "inverse_fc2.weight", "inverse_fc2.bias", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias",
            "bn1_next.weight", "bn1_next.bias")
    _SYM = "jh_icmnet_"
    F = 256            # feature size (icm.py:181)
    MAX_BATCH = 8192   # rows of one call (jh_icm.hip: kMaxBatch)

    def __init__(self, state_size, hidden, action_size, continuous, num_workers, max_batch, device, eta=0.01, gamma=0.99, obs_normalize=True, ri_normalize=True,
                 batch_norm=True, buckets=None):
        self._open(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.S, self.H, self.A, self.cont, self.W, self.maxB = int(state_size), int(hidden), int(action_size), bool(continuous), int(num_workers), int(max_batch)
        self.eta, self.gamma = float(eta), float(gamma)
        self.obs_normalize, self.ri_normalize, self.batch_norm = bool(obs_normalize), bool(ri_normalize), bool(batch_norm)
        n = int(self._fn("param_count_for")(self.S, self.H, self.A, int(self.cont), int(self.batch_norm)))
        if n <= 0:
            L.check(-2)
        self.n_params = n
        self.params, self.grads, self.m, self.v = self._zeros(n, 4) if buckets is None else buckets
        assert all(t.numel() == n and t.is_contiguous() and t.dtype == torch.float32 for t in (self.params, self.grads, self.m, self.v))
        flags = int(self.obs_normalize) | (int(self.ri_normalize) << 1) | (int(self.batch_norm) << 2)
        self.h = C.c_void_p()
        L.check(self._fn("create")(self.ctx, self.S, self.H, self.A, int(self.cont), self.W, self.maxB, flags, self.eta, self.gamma, L.ptr(self.params), L.ptr(self.grads),
                                   L.ptr(self.m), L.ptr(self.v), C.byref(self.h)))
        names = self._SEG[: int(self._fn("segment_count")(self.h))]
        assert len(names) == (18 if self.batch_norm else 12)
        self.seg = self._segments(names)
        self.stats_floats = int(self._fn("stats_floats")(self.h))
        self.ac = self.A if self.cont else 1

    def _pairs(self, bucket):
        """[(reference key, view of the bucket shaped like the reference tensor)] in the reference's registration order."""
        out = []
        for name, (off, rows, cols) in self.seg.items():
            v = bucket[off : off + rows * cols]
            out.append((name, v.view(rows, cols) if name.endswith(".weight") and not name.startswith("bn") else v))
        return out

    def export_state(self, bucket=None):
        return _export_pairs(self._pairs(self.params if bucket is None else bucket))

    def import_state(self, sd, bucket=None):
        _import_pairs(self._pairs(self.params if bucket is None else bucket), sd, self.device)

    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0):
        L.check(self._fn("set_hyper")(self.h, float(lr), float(beta1), float(beta2), float(eps), int(step), L.stream_ptr()))

    def set_lr(self, lr):
        L.check(self._fn("set_lr")(self.h, float(lr), L.stream_ptr()))

    def _stats_layout(self):
        S, H, W, F = self.S, self.H, self.W, self.F
        return (("rms_obs.mean", S), ("rms_obs.var", S), ("rms_obs.count", 0), ("rms_ri.mean", 1), ("rms_ri.var", 1), ("rms_ri.count", 0), ("rff.rewems", W),
                ("bn1.running_mean", H), ("bn1.running_var", H), ("bn2.running_mean", F), ("bn2.running_var", F), ("bn1_next.running_mean", H),
                ("bn1_next.running_var", H))

    def stats(self):
        """The statistics block as {reference state_dict key: float32 numpy array} (synchronises).  The batch norms' entries are there
        whether or not batch_norm is on (a module without batch norm has no such keys: the caller drops them)."""
        h = np.empty(self.stats_floats, np.float32)
        L.check(self._fn("stats_get")(self.h, L.ptr(h), L.stream_ptr()))
        out, o = {}, 0
        for name, k in self._stats_layout():
            out[name] = h[o : o + max(k, 1)].copy().reshape(() if k == 0 else (k,))
            o += max(k, 1)
        assert o == self.stats_floats
        return out

    def set_stats(self, d):
        """Entries of `d` (keys as stats()) replace the block's; the others stay (synchronises)."""
        cur = self.stats()
        for k, v in d.items():
            if k in cur:
                v = (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)).astype(np.float32)
                if v.size != cur[k].size:
                    raise ValueError(f"{k}: expected {cur[k].size} values, got {v.size}")
                cur[k] = v.reshape(cur[k].shape)
        h = np.concatenate([cur[name].reshape(-1) for name, _ in self._stats_layout()]).astype(np.float32)
        L.check(self._fn("stats_set")(self.h, L.ptr(h), L.stream_ptr()))

    def _check_rows(self, state, next_state, action):
        for t, w in ((state, self.S), (next_state, self.S), (action, self.ac)):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device and t.numel() == int(state.shape[0]) * w

    def obs_update(self, next_state):
        """icm.update_rms_obs(next_state) (icm_ppo.py:98)."""
        assert next_state.is_contiguous() and next_state.dtype == torch.float32 and next_state.shape[1] == self.S
        L.check(self._fn("obs_update")(self.h, L.ptr(next_state), int(next_state.shape[0]), L.stream_ptr()))

    def reward(self, state, next_state, action, reward, extrinsic_coeff=1.0, intrinsic_coeff=1.0, ri_mean=None, ri_raw=None, ri=None):
        """The no-grad pass of icm_ppo.py:99-102 over the whole rollout: `reward` [M] becomes ext * reward + int * r_i in place; optional outputs
        ri_mean [1], ri_raw [M] (before the normalisation), ri [M] (after)."""
        M = int(state.shape[0])
        self._check_rows(state, next_state, action)
        assert reward.is_contiguous() and reward.dtype == torch.float32 and reward.numel() == M
        assert (ri_raw is None or ri_raw.numel() == M) and (ri is None or ri.numel() == M) and (ri_mean is None or ri_mean.numel() >= 1)
        L.check(self._fn("reward")(self.h, L.ptr(state), L.ptr(next_state), L.ptr(action), M, float(extrinsic_coeff), float(intrinsic_coeff), L.ptr(reward), L.ptr(ri_mean),
                                   L.ptr(ri_raw), L.ptr(ri), L.stream_ptr()))

    def update(self, state, next_state, action, idx, beta, max_norm, stats=None, b=None):
        """One minibatch (icm_ppo.py:177, 185, 194-199) on rows idx (int64) of the rollout arrays, or on rows 0 .. b - 1.  stats [4] = l_f, l_i, 0, mark."""
        self._check_rows(state, next_state, action)
        b = int(idx.numel()) if idx is not None else (int(state.shape[0]) if b is None else int(b))
        assert idx is None or (idx.is_contiguous() and idx.dtype == torch.int64 and idx.device == self.device)
        assert stats is None or stats.numel() >= 4
        L.check(self._fn("update")(self.h, L.ptr(state), L.ptr(next_state), L.ptr(action), L.ptr(idx), b, int(state.shape[0]), float(beta),
                                   float(max_norm if max_norm else 0.0), L.ptr(stats), L.stream_ptr()))


class RNDNet(_NetObject):
    """jh_rndnet_*: RND-PPO's distillation module (network/rnd.py:173-225) -- predictor and frozen target, each fc1 -> bn1 -> ReLU -> fc2 -> bn2
    -> ReLU under batch statistics, the running moments of observations and intrinsic reward, the reward filter -- with the no-grad reward
    pass over a rollout (`obs_update`, `reward`) and one minibatch update of the predictor (`update`) as tile-engine launches plus the kernels
    of jh_rnd.hip / jh_curiosity.h.  The 16 tensors live in flat buckets, the predictor's eight first (`_SEG`; only they get gradients, moments
    and Adam steps); `_pairs` lists them in the reference's registration order (`_ORDER`).  Everything that is a buffer-like Parameter in the
    reference (rms_obs, rms_ri, rff, the batch norms' running statistics) lives in the device statistics block (`stats()` / `set_stats()`)."""

    _SEG = tuple(f"{layer}_{net}_mlp.{t}" for net in ("predict", "target") for layer in ("fc1", "fc2", "bn1", "bn2") for t in ("weight", "bias"))
    _ORDER = tuple(f"{kind}{i}_{net}_mlp.{t}" for kind in ("fc", "bn") for net in ("predict", "target") for i in (1, 2) for t in ("weight", "bias"))
    _SYM = "jh_rndnet_"
    F = 256            # feature size (rnd.py:196)
    MAX_BATCH = 8192   # rows of one call (jh_curiosity.h: kCurMaxBatch)

    def __init__(self, state_size, hidden, num_workers, max_batch, device, gamma_i=0.99, obs_normalize=True, ri_normalize=True, batch_norm=True, buckets=None):
        self._open(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.S, self.H, self.W, self.maxB = int(state_size), int(hidden), int(num_workers), int(max_batch)
        self.gamma_i = float(gamma_i)
        self.obs_normalize, self.ri_normalize, self.batch_norm = bool(obs_normalize), bool(ri_normalize), bool(batch_norm)
        n = int(self._fn("param_count_for")(self.S, self.H, int(self.batch_norm)))
        if n <= 0:
            L.check(-2)
        self.n_params = n
        self.params, self.grads, self.m, self.v = self._zeros(n, 4) if buckets is None else buckets
        assert all(t.numel() == n and t.is_contiguous() and t.dtype == torch.float32 for t in (self.params, self.grads, self.m, self.v))
        flags = int(self.obs_normalize) | (int(self.ri_normalize) << 1) | (int(self.batch_norm) << 2)
        self.h = C.c_void_p()
        L.check(self._fn("create")(self.ctx, self.S, self.H, self.W, self.maxB, flags, self.gamma_i, L.ptr(self.params), L.ptr(self.grads), L.ptr(self.m), L.ptr(self.v),
                                   C.byref(self.h)))
        assert int(self._fn("segment_count")(self.h)) == len(self._SEG)
        self.seg = {k: v for k, v in self._segments(self._SEG).items() if v[1] * v[2] > 0}  # without batch norm its segments are empty
        self.n_train = int(self._fn("trainable_floats")(self.h))
        self.stats_floats = int(self._fn("stats_floats")(self.h))

    def _pairs(self, bucket, trainable_only=False):
        """[(reference key, view of the bucket shaped like the reference tensor)] in the reference's registration order."""
        out = []
        for name in self._ORDER:
            if name not in self.seg or (trainable_only and "target" in name):
                continue
            off, rows, cols = self.seg[name]
            v = bucket[off : off + rows * cols]
            out.append((name, v.view(rows, cols) if name.endswith(".weight") and not name.startswith("bn") else v))
        return out

    def export_state(self, bucket=None):
        return _export_pairs(self._pairs(self.params if bucket is None else bucket))

    def import_state(self, sd, bucket=None):
        _import_pairs(self._pairs(self.params if bucket is None else bucket), sd, self.device)

    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0):
        L.check(self._fn("set_hyper")(self.h, float(lr), float(beta1), float(beta2), float(eps), int(step), L.stream_ptr()))

    def set_lr(self, lr):
        L.check(self._fn("set_lr")(self.h, float(lr), L.stream_ptr()))

    def _stats_layout(self):
        S, H, W, F = self.S, self.H, self.W, self.F
        return (("rms_obs.mean", S), ("rms_obs.var", S), ("rms_obs.count", 0), ("rms_ri.mean", 1), ("rms_ri.var", 1), ("rms_ri.count", 0), ("rff.rewems", W),
                ("bn1_predict_mlp.running_mean", H), ("bn1_predict_mlp.running_var", H), ("bn2_predict_mlp.running_mean", F), ("bn2_predict_mlp.running_var", F),
                ("bn1_target_mlp.running_mean", H), ("bn1_target_mlp.running_var", H), ("bn2_target_mlp.running_mean", F), ("bn2_target_mlp.running_var", F))

    stats, set_stats = ICMNet.stats, ICMNet.set_stats  # the block's codec is the same: {reference state_dict key: float32 array} by `_stats_layout`

    def _check_rows(self, next_state):
        assert next_state.is_contiguous() and next_state.dtype == torch.float32 and next_state.device == self.device and next_state.dim() == 2 and next_state.shape[1] == self.S

    def obs_update(self, next_state):
        """rnd.update_rms_obs(next_state) (rnd_ppo.py:119)."""
        self._check_rows(next_state)
        L.check(self._fn("obs_update")(self.h, L.ptr(next_state), int(next_state.shape[0]), L.stream_ptr()))

    def reward(self, next_state, ri, ri_mean=None, ri_raw=None):
        """The no-grad pass of rnd_ppo.py:120 over the whole rollout: ri [M] = the (normalised) intrinsic reward; optional ri_mean [1], ri_raw [M]."""
        self._check_rows(next_state)
        M = int(next_state.shape[0])
        assert ri.is_contiguous() and ri.dtype == torch.float32 and ri.numel() == M
        assert (ri_raw is None or ri_raw.numel() == M) and (ri_mean is None or ri_mean.numel() >= 1)
        L.check(self._fn("reward")(self.h, L.ptr(next_state), M, L.ptr(ri), L.ptr(ri_mean), L.ptr(ri_raw), L.stream_ptr()))

    def update(self, next_state, idx, max_norm, stats=None, b=None):
        """One minibatch (rnd_ppo.py:251-252, 261-266) on rows idx (int64) of next_state, or on rows 0 .. b - 1.  stats [4] = r_i mean, 0, 0, mark."""
        self._check_rows(next_state)
        b = int(idx.numel()) if idx is not None else (int(next_state.shape[0]) if b is None else int(b))
        assert idx is None or (idx.is_contiguous() and idx.dtype == torch.int64 and idx.device == self.device)
        assert stats is None or stats.numel() >= 4
        L.check(self._fn("update")(self.h, L.ptr(next_state), L.ptr(idx), b, int(next_state.shape[0]), float(max_norm if max_norm else 0.0), L.ptr(stats), L.stream_ptr()))


class StagingRing:
    """jh_ring_*: bounded lock-free multi-producer / single-consumer ring of transitions in pinned host memory
    (the async Ape-X transport).  `produce` may be called from any number of actor threads (the GIL is released
    inside the C call); `drain` belongs to the learner thread.

    columns: list of (name, jh_dtype, elems, shape) -- pass `store.columns` to stage for a DeviceStore.
    device=None builds a host-only ring (pageable memory; `consume_host` only)."""

    def __init__(self, slots, columns, with_priority=False, device="cuda"):
        self.lib = L.load()
        self.columns = list(columns)
        self.names = [c[0] for c in columns]
        self.slots, self.with_priority = int(slots), bool(with_priority)
        ctx = None
        if device is not None:
            self.device = torch.device(device)
            ctx = L.ctx(self.device.index if self.device.index is not None else torch.cuda.current_device())
        descs = (L.ColDesc * len(columns))(*[L.ColDesc(int(c[1]), int(c[2])) for c in columns])
        self.h = C.c_void_p()
        L.check(self.lib.jh_ring_create(ctx, self.slots, len(columns), descs, int(self.with_priority), C.byref(self.h)))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.jh_ring_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def produce(self, cols, priorities=None, timeout_ms=10000):
        """cols: dict name -> numpy array [n, ...] (converted to the stored dtype); thread-safe.  Blocks while the
        ring is full -- slots come back when the LEARNER thread drains / reclaims -- for at most timeout_ms
        (JhError, nothing written); timeout_ms < 0 waits forever."""
        arrs, n = [], None
        for name, dt, elems, _ in self.columns:
            src = np.asarray(cols[name]).reshape(len(cols[name]), -1)
            a = np.ascontiguousarray(src, dtype=_NP_OF[dt])
            if dt == L.JH_I64 and src.dtype.kind == "f" and not np.array_equal(a, src):
                raise ValueError(f"column {name} is stored as int64 (its first batch was integer-typed) but this batch holds fractional values")
            assert a.shape[1] == elems, f"column {name}: expected {elems} elems, got {a.shape[1]}"
            n = a.shape[0] if n is None else n
            assert a.shape[0] == n
            arrs.append(a)
        p = None
        if self.with_priority:
            p = np.ascontiguousarray(priorities, dtype=np.float64).reshape(-1)
            assert p.size == n
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        L.check(self.lib.jh_ring_produce(self.h, int(n), ptrs, None if p is None else p.ctypes.data, int(timeout_ms)))
        return n

    def drain(self, store, tree=None, max_rows=0):
        """Learner thread: everything published so far -> `store` (DeviceStore) [+ leaves into `tree` (SumTree)]."""
        n = C.c_int64()
        L.check(self.lib.jh_ring_drain(self.h, store.h, tree.h if tree is not None else None, int(max_rows), L.stream_ptr(), C.byref(n)))
        return int(n.value)

    def reclaim(self, wait=False):
        """Learner thread: give the slots of completed drains back to the producers (drain() does this too)."""
        L.check(self.lib.jh_ring_reclaim(self.h, int(bool(wait))))

    def consume_host(self, max_rows=0):
        """-> (dict name -> numpy [n, elems], priorities float64[n]) of the rows published so far."""
        cap = self.slots if max_rows <= 0 else int(max_rows)
        outs = [np.empty((cap, elems), dtype=_NP_OF[dt]) for _, dt, elems, _ in self.columns]
        prio = np.empty(cap, np.float64)
        ptrs = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        n = C.c_int64()
        L.check(self.lib.jh_ring_consume_host(self.h, cap, ptrs, prio.ctypes.data, C.byref(n)))
        k = int(n.value)
        return {name: o[:k] for name, o in zip(self.names, outs)}, prio[:k]

    def stats(self):
        a, b, w = C.c_int64(), C.c_int64(), C.c_double()
        L.check(self.lib.jh_ring_stats(self.h, C.byref(a), C.byref(b), C.byref(w)))
        return {"produced": a.value, "drained": b.value, "producer_wait_ms": w.value}


def tgemm_dense(a, b, a_kcont=True, b_kcont=True, epi=0, bias=None, aux=None, rowsum=False, M=None, N=None, K=None):
    """jh_tgemm_dense: C = A (.) B on the grouped LDS-tiled fp32 MFMA engine (dense operand modes).
    a: [M, K] if a_kcont else [K, M];  b: [N, K] if b_kcont else [K, N]  (row-major, any row stride)."""
    lib = L.load()
    M = (a.shape[0] if a_kcont else a.shape[1]) if M is None else M
    K = (a.shape[1] if a_kcont else a.shape[0]) if K is None else K
    N = (b.shape[0] if b_kcont else b.shape[1]) if N is None else N
    assert a.stride(-1) == 1 and b.stride(-1) == 1 and a.dtype == b.dtype == torch.float32
    c = torch.empty(M, N, dtype=torch.float32, device=a.device)
    rs = torch.empty(M, dtype=torch.float32, device=a.device) if rowsum else None
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())  # row-strided views are fine: the stride is passed as lda / ldb
    L.check(lib.jh_tgemm_dense(L.ctx(a.device.index), int(M), int(N), int(K), pa, int(a.stride(0)), int(bool(a_kcont)), pb, int(b.stride(0)), int(bool(b_kcont)),
                               L.ptr(c), int(c.stride(0)), int(epi), L.ptr(bias), L.ptr(aux), int(aux.stride(0)) if aux is not None else 0, L.ptr(rs), L.stream_ptr()))
    return (c, rs) if rowsum else c


def tgemm_set_cfg(cfg=""):
    """jh_tgemm_set_cfg: per-call-site tile / split / XCD-order overrides of the tile engine (measurement and tests); "" = defaults."""
    L.check(L.load().jh_tgemm_set_cfg((cfg or "").encode()))


def tgemm_dense_group(a_list, b_list):
    """jh_tgemm_dense_group: C_j = A_j B_j^T for up to six same-shape problems (A_j [M, K], B_j [N, K], contiguous) as ONE grouped
    launch -- the shape of the value networks' forward launches (online and target trunks side by side)."""
    lib = L.load()
    n = len(a_list)
    M, K = a_list[0].shape
    N = b_list[0].shape[0]
    for a, b in zip(a_list, b_list):
        assert a.shape == (M, K) and b.shape == (N, K) and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype == torch.float32
    cs = [torch.empty(M, N, dtype=torch.float32, device=a_list[0].device) for _ in range(n)]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    L.check(lib.jh_tgemm_dense_group(L.ctx(a_list[0].device.index), n, int(M), int(N), int(K), arr(a_list), arr(b_list), arr(cs), L.stream_ptr()))
    return cs
