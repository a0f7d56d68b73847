"""ops.PinnedBuffer: device-mapped pinned host memory with its arm / wait protocol, at the smallest shapes that can go wrong.

A kernel writes its results straight into the buffer (`.dev`), the host arms the elements written last, waits for their arrival
(`wait`) and reads `.np`.  Every value is compared bit for bit with the same call writing plain device tensors read with `.cpu()`.
"""
import gc
import weakref

import numpy as np
import pytest
import torch

from tests.util import cu, npy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from jorldy_amd import ops as _ops

    return _ops


def _td_inputs(B=2, A=2):
    rng = np.random.default_rng(11)
    q, qt = cu(rng.standard_normal((B, A)).astype(np.float32)), cu(rng.standard_normal((B, A)).astype(np.float32))
    action, reward, done = cu(rng.integers(0, A, (B, 1)).astype(np.float32)), cu(rng.standard_normal((B, 1)).astype(np.float32)), cu(np.array([[0.0], [1.0]], np.float32))
    return q, qt, action, reward, done


def test_float32_statistics_arrive_bit_equal_on_the_current_and_on_another_stream(ops):
    args = _td_inputs()
    want = npy(ops.td_loss(*args, 0.99)[2])  # {loss, max_Q, mean_td, 0} through a plain device tensor
    buf = ops.PinnedBuffer((8,), np.float32, torch.device("cuda", torch.cuda.current_device()))
    assert buf.dev.dtype == torch.float32 and tuple(buf.dev.shape) == (8,) and buf.dev.data_ptr() == buf.dev_ptr.value
    assert not buf.np.any(), "a fresh buffer is zero-filled"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for stream in (None, side):
        buf.np[:] = 0
        buf.arm((3,))
        assert buf.np[3] == -1.0 and not buf.np[:3].any() and not buf.np[4:].any()
        with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
            ops.td_loss(*args, 0.99, stats=buf.dev)
        buf.wait((3,), what="td_loss", stream=stream)
        assert buf.np[:4].tobytes() == want.tobytes()
        assert not buf.np[4:].any()
    torch.cuda.synchronize()


@pytest.mark.parametrize("N", [1, 3])  # N = 1: the 8-byte minimum allocation (the float32 Q buffer is 4 bytes)
def test_int64_actions_arrive_equal(ops, N):
    logits = cu(np.random.default_rng(5 + N).standard_normal((N, 2, 1)).astype(np.float32))
    act0, q0, _ = ops.value_act(logits)
    dev = torch.device("cuda", torch.cuda.current_device())
    act, q = ops.PinnedBuffer((N,), np.int64, dev), ops.PinnedBuffer((N,), np.float32, dev)
    assert act.dev.dtype == torch.int64 and q.dev.dtype == torch.float32
    act.arm()
    assert (act.np == -1).all()
    ops.value_act(logits, out=(act.dev, q.dev))
    act.wait(what="value_act", timeout_s=ops.ACT_WAIT_S)
    # jh_value_act writes q first, a system-scope fence, the action last: once the actions have arrived q is in place too
    assert np.array_equal(act.np, npy(act0)) and q.np.tobytes() == npy(q0).tobytes()
    torch.cuda.synchronize()


def test_wait_raises_when_nothing_arrives(ops):
    buf = ops.PinnedBuffer((8,), np.float32)
    buf.arm((3,))
    with pytest.raises(RuntimeError, match="probe"):
        buf.wait((3,), what="probe", timeout_s=0.05)  # nothing was launched
    act = ops.PinnedBuffer((3,), np.int64)
    act.arm()
    act.np[0] = act.np[2] = 1
    with pytest.raises(RuntimeError, match="probe"):
        act.wait(what="probe", timeout_s=0.05)


def test_the_alias_keeps_the_allocation_alive_and_the_last_reference_frees_it(ops):
    args = _td_inputs()
    want = npy(ops.td_loss(*args, 0.99)[2])
    buf = ops.PinnedBuffer((8,), np.float32)
    block, dev = weakref.ref(buf._block), buf.dev
    del buf
    gc.collect()
    assert block() is not None
    ops.td_loss(*args, 0.99, stats=dev)  # the kernel writes the mapped block through the alias
    assert npy(dev)[:4].tobytes() == want.tobytes()
    torch.cuda.synchronize()
    gc.disable()  # the release below is reference counting's, not the cycle collector's
    try:
        del dev
        assert block() is None, "the allocation outlived the buffer and its alias"
    finally:
        gc.enable()
    fresh = ops.PinnedBuffer((8,), np.float32)  # the block above was released by reference counting; a fresh one works
    fresh.arm((3,))
    ops.td_loss(*args, 0.99, stats=fresh.dev)
    fresh.wait((3,), what="td_loss")
    assert fresh.np[:4].tobytes() == want.tobytes()
    torch.cuda.synchronize()
