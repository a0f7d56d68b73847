"""PPONet.ppo_update (the four-launch minibatch update) against a recording of its own results, BIT FOR BIT (tests/golden/ppo_update_bits.npz,
tools/gen_ppo_update_bits.py; the calls: tests/ppo_update_bits_cases.py).

The fixture was recorded at the commit in front of the one that shortened the dependent fetch chains inside the four kernels (hyper block and kernel
arguments fetched at entry, a row's head sums kept in registers, the discrete row's terms evaluated once, the bias corrections on a wave of their own,
head pointers fetched as one block).  None of that may move a bit: np.array_equal on the raw words, not a tolerance.

  a. every case of the table: three consecutive updates -> the four buckets, the three statistics rows, the hyper block (SHA-256 digests after every
     call; for the hidden-512 benchmark shape the digests alone)
  b. do_adam=False + adam_step (the data-parallel shape: norm kernel + plain Adam kernel)
  c. a captured update replayed three times = three eager calls = the fixture; the step counter advances by exactly one per update
  d. the same with the library's profiler repeating the idempotent launches 20 times
  e. a stand-alone update right after set_hyper(step=k)
"""
import numpy as np
import pytest
import torch

import ppo_update_bits_cases as BC
from tests.util import load

pytestmark = pytest.mark.gpu

JH_HY_STEP = 4


@pytest.fixture(scope="module")
def golden():
    g = load("ppo_update_bits")
    return {k: g[k] for k in g.files}


def _same_bits(got, golden, what):
    keys = [k for k in golden if k.startswith(what + "/")]
    assert keys and set(keys) == set(got), f"{what}: fixture keys {sorted(keys)} vs replayed {sorted(got)}"
    bad = []
    for k in sorted(keys):
        a, b = got[k], golden[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{k}: {a.shape} {a.dtype} vs fixture {b.shape} {b.dtype}"
        if not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            n = int((a.view(np.uint8) != b.view(np.uint8)).sum())
            bad.append(f"{k}: {n} bytes differ" + (f", max |diff| {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e}" if a.dtype == np.float32 else ""))
    assert not bad, f"{what}: not the recorded bits -- " + "; ".join(bad)


@pytest.mark.parametrize("c", BC.CASES, ids=BC.IDS)
def test_three_updates_same_bits(c, golden):
    _same_bits(BC.run_case(c), golden, c.name)


def test_no_adam_then_adam_step_same_bits(golden):
    _same_bits(BC.run_no_adam(), golden, "noadam_" + BC.CASES[0].name)


def test_update_after_set_hyper_same_bits(golden):
    got = BC.run_set_hyper(k=1000)
    name = "sethyper_" + BC.CASES[0].name
    assert list(got[name + "/hyper"][:, JH_HY_STEP]) == [1.0, 1001.0]
    _same_bits(got, golden, name)


@pytest.mark.parametrize("profiled", [False, True], ids=["plain", "lib_profile_x20"])
def test_captured_update_replayed_three_times(profiled, golden):
    """One update captured into a graph and replayed three times leaves what three eager calls leave (the fixture's first case), hyper block included;
    under the profiler the captured graph is replaced by eager calls whose idempotent launches repeat 20 times: the step still advances once per update."""
    from jorldy_amd import ops

    c = BC.CASES[0]
    d = BC.make_inputs(c)
    dev = BC.to_device(d)
    eager, other = BC.make_net(c, d), BC.make_net(c, d)
    st_e, st_o = torch.full((8,), -1.0, device="cuda"), torch.full((8,), -1.0, device="cuda")
    rec_e, rec_o = BC.Recorder(c.name, False), BC.Recorder(c.name, False)
    if profiled:
        ops.lib_profile(True, 20)
        try:
            for _ in range(BC.CALLS):
                BC.update(other, dev, st_o)
                rec_o.add(other, st_o)
        finally:
            ops.lib_profile(False)
    else:
        BC.update(other, dev, st_o)  # warm-up (first-use allocations), then back to the start
        other.params.copy_(torch.from_numpy(d["p0"]))
        other.m.zero_()
        other.v.zero_()
        other.set_hyper(BC.LR, BC.B1, BC.B2, BC.ADAM_EPS, step=0.0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.graph_capture(graph):
            BC.update(other, dev, st_o)
        for _ in range(BC.CALLS):
            graph.replay()
            rec_o.add(other, st_o)
    for _ in range(BC.CALLS):
        BC.update(eager, dev, st_e)
        rec_e.add(eager, st_e)
    got_o, got_e = rec_o.record(), rec_e.record()
    assert list(got_o[c.name + "/hyper"][:, JH_HY_STEP]) == [1.0, 2.0, 3.0], "the step counter must advance by exactly one per update"
    _same_bits(got_e, golden, c.name)
    _same_bits(got_o, golden, c.name)
