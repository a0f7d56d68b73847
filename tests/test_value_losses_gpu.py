"""jh_c51_loss and jh_td_loss against the float64 truths of tests/c51_truth.py and tests/td_truth.py over every dispatch edge of
csrc/jh_dqn.hip: the workgroup-per-sample and the wave-per-sample C51 kernels on both sides of B = 1024, one to four atoms per lane, the
block kernel's three-piece weight preload and its shuffled / direct reward loads, actions strided over waves, every flag combination, and
the inputs at which the loss has corners (probabilities under the 1e-8 clamp, mass dropped on exact atoms or outside the support, terminal
first steps, exact ties of the selector, actions out of range).

Criterion (tests/fp64_truth.py): |ours - exact| <= max(1e-5, 2 x |oracle32 - exact|) relative to max |exact|, per tensor, where oracle32 is
the numpy float32 oracle run on the truth's support.  tests/test_value_losses_cpu.py proves beforehand, on the CPU, that on every case the
oracle takes the truth's discrete decisions (l, u, a*) and that no row sits on a discontinuity, which is what makes the oracle's own error a
meaningful allowance.  Everything discrete is asserted exactly."""
import numpy as np
import pytest
import torch

import c51_truth as C
import fp64_truth as T
import td_truth as D
from test_value_losses_cpu import c51_case, c51_oracle32, td_case
from tests.util import f32, npy

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _vs(ours, exact, ref32, what):
    """The figures first, then the assertion (fp64_truth.vs_exact, which also enters them in the margin ledger)."""
    t64 = lambda a: torch.from_numpy(np.atleast_1d(np.asarray(a, dtype=np.float64)))
    o, e, r = t64(ours), t64(exact), t64(ref32)
    scale = float(e.abs().max()) + 1e-30
    print(f"{what}: |ours - fp64| / max = {float((o.reshape(e.shape) - e).abs().max()) / scale:.3e}, oracle32: {float((r.reshape(e.shape) - e).abs().max()) / scale:.3e}")
    return T.vs_exact(o, e, r, TOL, what)


def _opt(a):
    return None if a is None else f32(a)


def _run_c51(d):
    from jorldy_amd import ops

    g, prio, kl, st = ops.c51_loss(f32(d["logit"]), f32(d["target"]), f32(d["action"]), f32(d["reward"]), f32(d["done"]), C.V_MIN, C.V_MAX, C.GAMMA,
                                   next_logit_online=_opt(d["next_online"]), weights=_opt(d["weights"]), alpha=C.ALPHA, n_step=d["n_step"],
                                   stats=torch.full((8,), -1.0, device="cuda"))
    torch.cuda.synchronize()
    return npy(g), npy(prio), npy(kl), npy(st)


def _check_c51(tag, d, t, ro, out):
    g, prio, kl, st = out
    B, A, K = d["logit"].shape
    assert np.isfinite(g).all() and np.isfinite(kl).all() and np.isfinite(prio).all() and np.isfinite(st).all()
    _vs(g, t["grad"], ro["d_logit"], f"{tag} d(loss)/d(logit)")
    _vs(kl, t["kl"], ro["KL"], f"{tag} KL")
    _vs(prio, t["prio"], ro["prio"], f"{tag} priority")
    _vs(st[0], t["loss"], ro["loss"], f"{tag} loss")
    _vs(st[4], t["mean_kl"], ro["mean_kl"], f"{tag} mean KL")
    _vs(st[1], t["max_Q"], ro["max_Q"], f"{tag} max Q")
    assert st[2] == d["logit"].max() and st[3] == d["logit"].min(), "max / min logit are the input's, bit for bit"
    assert st[5] == 0.0 and st[6] == 0.0 and st[7] == 0.0
    act = np.clip(d["action"].astype(np.int64), 0, A - 1)
    other = np.ones((B, A), bool)
    other[np.arange(B), act] = False
    assert not g[other].any(), "gradient rows of the actions not taken are zeros"
    dropped = t["mass"] == 0
    assert not kl[dropped].any() and not prio[dropped].any() and not g[dropped].any(), "rows without projected mass: KL, priority and gradient are 0"
    assert (kl[~dropped] > 0).all()


@pytest.mark.parametrize("case", C.SWEEP, ids=[C.case_id(c) for c in C.SWEEP])
def test_c51_loss_matches_float64_truth_over_a_sweep(case):
    d, t, ro = c51_case(case)
    out = _run_c51(d)
    _check_c51(C.case_id(case), d, t, ro, out)
    if case[5] == "exact_tie":
        # the same call with the tie broken by hand: the later of the two identical selector rows gets all its mass on the lowest atom
        zn = d["next_online"].copy()
        tie = np.nonzero(t["gap"] == 0.0)[0]
        assert tie.size >= 1
        for b in tie:
            later = max(a for a in range(case[1]) if np.array_equal(zn[b, a], zn[b, t["a_star"][b]]))
            assert later != t["a_star"][b]
            zn[b, later] = 0.0
            zn[b, later, 0] = 30.0
        g2, prio2, kl2, st2 = _run_c51(dict(d, next_online=zn))
        assert np.array_equal(out[0], g2) and np.array_equal(out[1], prio2) and np.array_equal(out[2], kl2) and np.array_equal(out[3], st2), "the first of two identical rows wins"


def test_c51_block_kernel_and_wave_kernel_agree_row_by_row():
    """B = 1025 takes the wave-per-sample kernel, its first 1024 rows alone the workgroup-per-sample kernel: per-row KL and priority do not
    depend on the batch and are bit-identical (the source's claim); the gradients differ by the two calls' (mean weight / B) only."""
    d, t, ro = c51_case(C.BLOCK_VS_WAVE)
    B = C.BLOCK_VS_WAVE[0]
    assert B == 1025 and d["weights"] is not None
    head = {k: (v[:1024] if isinstance(v, np.ndarray) else v) for k, v in d.items()}
    t_head = C.truth_of(head)
    ro_head = c51_oracle32(head, t_head)
    g, prio, kl, st = _run_c51(d)
    g_h, prio_h, kl_h, st_h = _run_c51(head)
    assert np.array_equal(kl[:1024], kl_h) and np.array_equal(prio[:1024], prio_h)
    _check_c51("first 1024 rows", head, t_head, ro_head, (g_h, prio_h, kl_h, st_h))
    w = d["weights"].astype(np.float64)
    rescale = (w[:1024].mean() / 1024.0) / (w.mean() / 1025.0)
    _vs(g[:1024].astype(np.float64) * rescale, t_head["grad"], ro_head["d_logit"], "wave kernel's rows 0..1023, rescaled, d(loss)/d(logit)")


def _run_td(d):
    from jorldy_amd import ops

    g, prio, st = ops.td_loss(f32(d["q"]), f32(d["q_next_target"]), f32(d["action"]), f32(d["reward"]), f32(d["done"]), D.GAMMA, q_next_online=_opt(d["q_next_online"]),
                              weights=_opt(d["weights"]), alpha=D.ALPHA, n_step=d["n_step"], stats=torch.full((4,), -1.0, device="cuda"))
    torch.cuda.synchronize()
    return npy(g), npy(prio), npy(st)


@pytest.mark.parametrize("case", D.SWEEP, ids=[D.case_id(c) for c in D.SWEEP])
def test_td_loss_matches_float64_truth_over_a_sweep(case):
    d, t, ro = td_case(case)
    tag = D.case_id(case)
    g, prio, st = _run_td(d)
    B, A = d["q"].shape
    assert np.isfinite(g).all() and np.isfinite(prio).all() and np.isfinite(st).all()
    _vs(g, t["grad"], ro["d_q_all"], f"{tag} d(loss)/d(q)")
    _vs(prio, t["prio"], ro["prio"], f"{tag} priority")
    _vs(st[0], t["loss"], ro["loss"], f"{tag} loss")
    _vs(st[1], t["max_Q"], ro["max_Q"], f"{tag} max Q")
    _vs(st[2], t["mean_td"], ro["mean_td"], f"{tag} mean td")
    assert st[3] == 0.0
    act = np.clip(d["action"].astype(np.int64), 0, A - 1)
    other = np.ones((B, A), bool)
    other[np.arange(B), act] = False
    assert not g[other].any(), "the gradient is zero off the taken action"
    zero = t["td"] == 0
    assert not prio[zero].any() and not g[zero].any(), "rows with td exactly 0"
