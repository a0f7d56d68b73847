import numpy as np
import torch

from ... import ops
from .base import h2d_small
from .replay_buffer import ReplayBuffer


class PERBuffer(ReplayBuffer):
    """core/buffer/per_buffer.py:7-105 on the GPU.

    The float64 sum tree lives in HBM (array-heap layout, 2N-1 nodes, leaves at [N-1, 2N-2]); store,
    priority write-back and sampling are batch kernels that reproduce the reference's sequential
    `+= delta` arithmetic per node, so tree contents and sampled indices are bit-identical.  The
    three numpy global-RNG draws of `sample` stay on the host, in the reference's order.
    """

    def __init__(self, buffer_size, uniform_sample_prob=1e-3, device=None, frame_dedup=False, frame_pool_factor=2.0):
        super().__init__(buffer_size, device, frame_dedup=frame_dedup, frame_pool_factor=frame_pool_factor)
        self.tree_size = self.buffer_size * 2 - 1
        self.first_leaf_index = self.buffer_size - 1
        self.uniform_sample_prob = uniform_sample_prob
        self._tree = ops.SumTree(self.buffer_size, uniform_sample_prob, device=self.device)
        self._next_prio = None
        self._shards = None  # (dist, group) when this buffer is one shard of a data-parallel logical buffer

    # -- store ------------------------------------------------------------------------------------
    def store_soa(self, cols, priorities=None):
        cols = {k: v for k, v in cols.items() if k != "priority"}
        self._next_prio = None if priorities is None else np.array(priorities, dtype=np.float64, copy=True).reshape(-1)
        n = super().store_soa(cols)
        if not self._was_deferred:  # rows are in HBM, leaves follow now
            self._tree.push(n, self._next_prio)   # per_buffer.py:27-33 (max_priority when no actor-side priority)
        return n

    def store_device(self, cols, example=None, priorities=None):
        """+ the rows' leaves; `priorities`: host values, or a float64 CUDA tensor [n] (actor-side priorities computed on the device)."""
        n = super().store_device(cols, example)
        if torch.is_tensor(priorities):
            self._tree.push_device(n, priorities)
        else:
            self._tree.push(n, None if priorities is None else np.asarray(priorities, dtype=np.float64).reshape(-1))
        return n

    def store_feed_rows(self, cols, n, priorities=None):
        """+ the rows' leaves: actor-side priorities (float64, device) or max_priority (per_buffer.py:25-30)."""
        super().store_feed_rows(cols, n)
        if priorities is None:
            self._tree.push(n, None)
        else:
            self._tree.push_device(n, priorities)
        return n

    def _defer(self, flat, n, extra=None):
        super()._defer(flat, n, self._next_prio)

    def flush(self):
        """Held rows -> ring, then their leaves in the same order.  Rows without an actor-side priority take
        max_priority, which cannot have changed since they were stored: every priority update flushes first."""
        done = self._flush_rows()
        i = 0
        while i < len(done):  # one tree push per run of the same kind (with / without explicit priorities)
            j, n = i, 0
            has = done[i][1] is not None
            while j < len(done) and (done[j][1] is not None) == has:
                n += done[j][0]
                j += 1
            self._tree.push(n, (done[i][1] if j == i + 1 else np.concatenate([d[1] for d in done[i:j]])) if has else None)
            i = j

    def store(self, transitions):
        if self.first_store:
            self.check_dim(transitions[0])
        if not transitions:
            return
        prio = None
        if "priority" in transitions[0]:  # Ape-X actor-side priorities (ape_x.py:188-196), (1,1) arrays
            prio = np.asarray([np.asarray(t["priority"]).reshape(-1)[0] for t in transitions], dtype=np.float64)
        self.store_soa(self.stack_transition(transitions, skip=("priority",)), prio)

    def _drain_tree(self):
        return self._tree  # drained rows get their leaves in the same call (actor priorities or max_priority)

    # -- priorities -------------------------------------------------------------------------------
    def update_priorities(self, indices, priorities):
        """Batched write-back: indices int64 device tensor (tree space), priorities float32/float64
        device tensor; equivalent to `for i, p in zip(indices, p_j): update_priority(p.item(), i)`
        (per.py:69-70, rainbow.py:230-231) without the B host syncs."""
        self.flush()
        self._tree.update(indices.reshape(-1), priorities.reshape(-1))

    def update_priority(self, new_priority, index):
        """Scalar compatibility path (per_buffer.py:42-48)."""
        self.flush()
        idx = h2d_small(np.asarray([index], dtype=np.int64), self.device)
        p = h2d_small(np.asarray([float(np.asarray(new_priority).reshape(-1)[0])], dtype=np.float64), self.device)
        self._tree.update(idx, p)

    # -- sample -----------------------------------------------------------------------------------
    def draw(self, batch_size):
        """per_buffer.py:72-81: the three global-RNG draws, in reference order."""
        mask = np.random.uniform(size=batch_size) < self.uniform_sample_prob
        n_uni = int(np.sum(mask))
        uni = np.random.randint(self.buffer_counter, size=n_uni)
        u = np.random.uniform(size=batch_size - n_uni)
        return uni, u

    def attach_shards(self, dist, group=None, transport=None):
        """Data-parallel learners (jorldy_amd.parallel.attach_data_parallel): this rank's buffer becomes one shard of
        a logical buffer of world_size x buffer_size slots; sampling stays local, the IS weights are normalised over
        the global batch against the global root / count (parallel.sharded_is_weights)."""
        if transport is None:
            from ...parallel import Transport

            transport = Transport(dist, group, self.device)
        self._shards = (dist, group, transport)

    def _global_weights(self, beta, idx, w_out, stats):
        """parallel.sharded_is_weights (the reference form, used by the gloo test) as two small kernels around ONE
        all-gather of 3 float64 per rank: jh_per_shard_stats -> all_gather -> jh_per_weights_sharded."""
        dist, group, transport = self._shards
        G = transport.world
        if getattr(self, "_shard_bufs", None) is None or self._shard_bufs[1].numel() != 3 * G:
            self._shard_bufs = (torch.zeros(3, dtype=torch.float64, device=self.device), torch.zeros(3 * G, dtype=torch.float64, device=self.device))
        loc, allv = self._shard_bufs
        B = int(idx.numel())
        self._tree.shard_stats(B, loc)
        if G > 1:
            transport.all_gather_f64_(allv, loc)
        else:
            allv.copy_(loc)
        self._tree.weights_sharded(B, beta, allv, w_out)

    def sample_into(self, beta, batch_size, idx_out, w_out):
        """Host RNG draws (reference order) + descent / IS weights into PREALLOCATED idx / weight tensors;
        the gather is left to the caller (captured-graph learners).  Returns the stats tensor
        {sampled_p, mean_p, root, max_w}."""
        assert self.buffer_counter > 0
        self.flush()
        uni, u = self.draw(batch_size)
        _, _, _, stats = self._tree.sample(beta, uni, u, want_w64=False, out_idx=idx_out, out_w32=w_out)
        if self._shards is not None:
            self._global_weights(beta, idx_out, w_out, stats)
        return stats

    def sample(self, beta, batch_size, as_float=True):
        """-> (transitions, weights f32[B] device, indices i64[B] device (tree space, uniform first),
               sampled_p, mean_p) ; sampled_p/mean_p are 0-dim device float64 tensors (call .item()
               when logging)."""
        assert self.buffer_counter > 0
        self.flush()
        uni, u = self.draw(batch_size)
        idx, w64, w32, stats = self._tree.sample(beta, uni, u, want_w64=False)
        if self._shards is not None:
            self._global_weights(beta, idx, w32, stats)
        transitions = self.gather(idx, idx_offset=self.first_leaf_index, as_float=as_float)
        stats = stats.clone()
        return transitions, w32, idx, stats[0], stats[1]

    # -- complete checkpoints --------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()  # flushes
        st = self._tree.state()
        sd.update({"sum_tree": self._tree.dump(), "max_priority": st["max_priority"], "tree_index": st["tree_index"]})
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self._next_prio = None
        self._tree.load(sd["sum_tree"], sd["max_priority"], sd["tree_index"], sd["buffer_counter"])

    def save_stream(self, dirpath):
        import os

        meta = super().save_stream(dirpath)
        st = self._tree.state()
        self._tree.dump().tofile(os.path.join(dirpath, "sum_tree.f64"))
        meta.update({"sum_tree": "sum_tree.f64", "max_priority": st["max_priority"], "tree_index": st["tree_index"]})
        return meta

    def load_stream(self, dirpath, meta):
        import os

        super().load_stream(dirpath, meta)
        tree = np.fromfile(os.path.join(dirpath, meta["sum_tree"]), dtype=np.float64)
        self._next_prio = None
        self._tree.load(tree, meta["max_priority"], meta["tree_index"], meta["buffer_counter"])

    # -- state the reference exposes ----------------------------------------------------------------
    @property
    def sum_tree(self):
        self.flush()
        return self._tree.dump()

    @property
    def max_priority(self):
        self.flush()
        return self._tree.state()["max_priority"]

    @property
    def tree_index(self):
        self.flush()
        return self._tree.state()["tree_index"]
