"""The float64 truth of one PPO minibatch update (tests/fp64_truth.py: ppo_update_float64) and the input generator of the
jh_pponet_ppo_update_rows sweep (tests/ppo_update_cases.py), checked without a GPU."""
import numpy as np
import pytest
import torch

import fp64_truth as T
import ppo_update_cases as PC


@pytest.mark.parametrize("c", PC.CASES, ids=PC.IDS)
def test_generated_inputs_keep_the_float64_truth_well_defined(c):
    """Every case of the sweep: no row near a kink of the loss, the critic's branch pinned (or both branches' gradients equal), both sides of
    every min / max populated -- with no row excluded (conditions on the reference alone, see ppo_update_cases)."""
    inp = PC.make(c)
    shares = PC.check_conditions(c, inp, PC.truth(c, inp))
    print(PC.case_id(c), shares)
    again = PC.make(c)  # deterministic per case: the GPU legs regenerate the same inputs
    assert all(torch.equal(inp[k], again[k]) for k in ("x", "action", "adv", "ret", "value_old", "logp_old"))


def test_the_table_has_every_boundary_of_the_dispatch():
    """The list the sweep must contain at least once each (B boundaries with both policy kinds)."""
    has = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in PC.CASES)
    for B in (1, 255, 1023, 1024, 1025, 2047, 2048, 2049, 16384, 16385):
        assert has(B=B, cont=True) and has(B=B, cont=False), B
    assert any(c.B > 16384 and c.B % 256 for c in PC.CASES if c.cont) and any(c.B > 16384 and c.B % 256 for c in PC.CASES if not c.cont)
    for H, B in ((16, 1041), (32, 1027), (64, 1030), (128, 1025), (64, 4101)):
        assert has(H=H, B=B, regime="tail", cont=True) and has(H=H, B=B, regime="tail", cont=False), (H, B)
        assert (B * (H // 4)) % 64 != 0
    assert {c.H for c in PC.CASES} >= {16, 32, 48, 64, 128, 512} and all(c.B <= 2049 for c in PC.CASES if c.H == 512)
    n_out = lambda c: 2 * c.A + 1 if c.cont else c.A + 1
    assert {n_out(c) for c in PC.CASES if c.B > 1024} >= {3, 7, 8, 9, 13, 17}
    assert any(c.H < (n_out(c) + 3) // 4 * 4 and n_out(c) > 8 and c.B > 1024 for c in PC.CASES if c.H == 16) and any(c.H < (n_out(c) + 3) // 4 * 4 and c.B > 1024 for c in PC.CASES if c.H == 32)
    assert {c.S for c in PC.CASES} >= {3, 4, 8, 9, 11, 16, 17, 27}
    assert any(c.M == 0 for c in PC.CASES) and any(c.M > c.B for c in PC.CASES)
    assert {c.max_norm for c in PC.CASES} >= {0.0, 1e-4, 0.5, 1e4}
    assert {c.regime for c in PC.CASES} == {"c1", "c2", "own", "tail"}


@pytest.mark.parametrize("cont,S,H,A,B", [(False, 4, 32, 3, 40), (True, 5, 16, 2, 33)])
def test_ppo_update_float64_equals_the_head_gradients_composed_by_hand(cont, S, H, A, B):
    """ppo_update_float64 = ppo_head_grads_float64 (d loss / d raw heads from given head values) pushed through the mirror module's raw() by hand."""
    c = PC.Case(cont, S, H, A, B, 2 * B, "c1", 0.5)
    inp = PC.make(c)
    heads, stats, grads, rows = PC.truth(c, inp)
    r = PC.gathered(inp)
    names = ("mu_raw", "log_std_raw", "v") if cont else ("logits", "v")
    hg = T.ppo_head_grads_float64(cont, {k: h.numpy() for k, h in zip(names, heads)}, r["action"].numpy(), r["adv"].numpy(), r["ret"].numpy(), r["value_old"].numpy(),
                                  r["logp_old"].numpy(), inp["eps"], inp["vf"], inp["ent"])
    module = inp["module"]
    for p in module.parameters():
        p.grad = None
    out = module.raw(r["x"].double())
    torch.autograd.backward(list(out), [torch.from_numpy(hg[k]).reshape(o.shape) for k, o in zip(names, out)])
    for k, p in module.named_parameters():
        np.testing.assert_allclose(grads[k].numpy(), p.grad.numpy(), rtol=1e-12, atol=1e-14 * float(p.grad.abs().max()), err_msg=k)
    np.testing.assert_allclose(rows["ratio"].numpy(), hg["ratio"].reshape(-1), rtol=1e-13)
    assert stats["critic"] == max(stats["c1"], stats["c2"]) and stats["max_ratio"] == float(rows["ratio"].max())
    # ... and the float32 comparator is the same function on as32(module)
    h32, s32, g32, _ = PC.truth(c, inp, T.as32(module))
    assert all(g.dtype == torch.float32 for g in g32.values()) and abs(s32["loss"] - stats["loss"]) <= 1e-5 * (1 + abs(stats["loss"]))
