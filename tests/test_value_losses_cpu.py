"""CPU-side checks behind tests/test_value_losses_gpu.py: the float64 truths of tests/c51_truth.py and tests/td_truth.py reproduce the
reference's own learn() on the fixtures, the truth's default support is torch.linspace up to the last bit, and every case of the two sweeps
satisfies the conditions under which `|ours - exact| <= max(1e-5, 2 x |oracle32 - exact|)` is a meaningful criterion: the float32 oracle,
run on the truth's support, takes the same discrete decisions (l, u, a*) as the truth on every row, and no row sits on a discontinuity
(a near-tie of the selector, a probability at the 1e-8 clamp, a projected mass at the 1e-8 floor, |td| at Huber's kink)."""
import functools

import numpy as np
import pytest

import c51_truth as C
import td_truth as D
from oracle import jorldy_oracle as O
from tests.util import load


def _h(z, k):
    return z[f"hyper/{k}"].item()


def _target_logit_from_p(p):
    return np.log(np.maximum(p, 1e-30)).astype(np.float32)  # the fixtures hold the target net's probabilities; softmax(log p) = p


def _logit_with_q_order(q, K):
    """[B, A] expected values -> [B, A, K] logits with the same ordering (the fixture records next_q_action, not the logits behind it)."""
    B, A = q.shape
    out = np.full((B, A, K), -30.0, np.float32)
    order = np.argsort(np.argsort(q, axis=1), axis=1)
    for b in range(B):
        for a in range(A):
            out[b, a, order[b, a]] = 30.0
    return out


# ----------------------------------------------------------------------------------------------- the float32 comparators of the sweeps
def c51_oracle32(d, t):
    """oracle.c51_project_kl on a sweep case, on the truth's support.  The oracle indexes with the action as it comes: it gets the clipped one.
    -> its result, with the priorities and the mean KL formed in float32 for the cases without weights too."""
    B, A, K = d["logit"].shape
    n = d["reward"].shape[1]
    act = np.clip(d["action"].astype(np.int64), 0, A - 1)
    ro = O.c51_project_kl(d["logit"], act, d["reward"].reshape(B, n, 1), d["done"].reshape(B, n, 1), d["target"], C.V_MIN, C.V_MAX, K, C.GAMMA,
                          next_logit_online=d["next_online"], weights=d["weights"], alpha=C.ALPHA, support=t["support"])
    ro["prio"] = np.power(ro["KL"], np.float32(C.ALPHA))
    ro["mean_kl"] = ro["KL"].mean(dtype=np.float32)
    return ro


def td_oracle32(d):
    B, A = d["q"].shape
    n = d["reward"].shape[1]
    act = np.clip(d["action"].astype(np.int64), 0, A - 1)
    shape = (B, n, 1) if d["n_step"] else (B, 1)
    ro = O.dqn_loss(d["q"], act, d["reward"].reshape(shape), d["done"].reshape(shape), d["q_next_target"], D.GAMMA, next_q_online=d["q_next_online"],
                    weights=d["weights"], alpha=D.ALPHA, n_step=d["n_step"])
    ro["prio"] = (ro["p_j"] if ro["p_j"] is not None else ro["td_error"]).reshape(B)
    ro["mean_td"] = ro["td_error"].mean(dtype=np.float32)
    return ro


@functools.lru_cache(maxsize=None)
def c51_case(case):
    """-> (inputs, float64 truth, float32 oracle on the truth's support), computed once per session and read-only afterwards."""
    d = C.sweep_case(*case)
    t = C.truth_of(d)
    return d, t, c51_oracle32(d, t)


@functools.lru_cache(maxsize=None)
def td_case(case):
    d = D.sweep_case(*case)
    return d, D.truth_of(d), td_oracle32(d)


# ----------------------------------------------------------------------------------------------- the truths against the reference
def _c51_fixture_inputs(name):
    z = load(name)
    B, A, K = int(_h(z, "B")), int(_h(z, "A")), int(_h(z, "num_support"))
    kw = dict(logit=z["learn/logit"].reshape(B, A, K), target=_target_logit_from_p(z["learn/target_p_logit"]), action=z["learn/action"],
              v_min=_h(z, "v_min"), v_max=_h(z, "v_max"), gamma=_h(z, "gamma"))
    if name == "c51":
        np.random.seed(int(_h(z, "np_seed")))
        rows = np.random.randint(z["buf_state"].shape[0], size=B)
        kw.update(next_online=None, reward=z["buf_reward"][rows], done=z["buf_done"][rows], weights=None, alpha=1.0)
    else:
        kw.update(next_online=_logit_with_q_order(z["learn/next_q_action"], K), reward=z["learn/reward"], done=z["learn/done"], weights=z["learn/weights"],
                  alpha=_h(z, "alpha"))
    return z, kw


@pytest.mark.parametrize("name", ["c51", "rainbow"])
def test_c51_truth_reproduces_the_reference_fixture(name):
    """Tolerances: those of test_c51_fixture / test_rainbow_fixture (tests/test_kernels_gpu.py) for the same arrays."""
    z, kw = _c51_fixture_inputs(name)
    t = C.c51_truth(**kw)
    B = t["kl"].size
    np.testing.assert_allclose(t["loss"], z["learn/loss"], rtol=1e-5)
    np.testing.assert_allclose(t["max_Q"], z["result/max_Q"], rtol=1e-5)
    np.testing.assert_allclose(t["max_logit"], z["result/max_logit"], rtol=1e-6)
    np.testing.assert_allclose(t["min_logit"], z["result/min_logit"], rtol=1e-6)
    np.testing.assert_allclose(t["grad"].reshape(z["learn/d_logit"].shape), z["learn/d_logit"], rtol=1e-4, atol=1e-8)
    if name == "rainbow":
        np.testing.assert_allclose(t["kl"], z["learn/KL"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(t["prio"], z["learn/p_j"], rtol=1e-5, atol=1e-6)
    assert np.array_equal(t["a_star"], z["learn/target_action"].reshape(B))
    # the discrete decisions: the recorded l / u, and the atoms that carry mass in the recorded target distribution
    assert np.array_equal(t["l"], z["learn/l"]) and np.array_equal(t["u"], z["learn/u"])
    assert np.array_equal(t["target_dist"] > 0, z["learn/target_dist"] > 0)
    np.testing.assert_allclose(t["target_dist"], z["learn/target_dist"], rtol=1e-5, atol=1e-6)
    assert int(C.near_ties(t).sum()) == 0 and int((t["clamp_dist"] < 0.5).sum()) == 0


def _td_fixture(name):
    z = load(name)
    B, A = int(_h(z, "B")), int(_h(z, "A"))
    a = z["learn/action"].astype(np.int64).reshape(B)
    q = np.zeros((B, A), np.float32)  # the fixture records the taken action's Q only: that is all the loss reads
    q[np.arange(B), a] = z["learn/q"].reshape(B)
    double = name in ("double", "per", "ape_x")
    per = name in ("per", "ape_x")
    n_step = int(_h(z, "n_step")) if name in ("multistep", "ape_x") else 0
    if n_step:
        r, d = z["learn/reward"], z["learn/done"]
    elif per:
        leaf = z["learn/indices"] - ((z["tree0"].shape[0] + 1) // 2 - 1)
        r, d = z["buf_reward"][leaf], z["buf_done"][leaf]
    else:
        np.random.seed(int(_h(z, "np_seed")))
        rows = np.random.randint(z["buf_state"].shape[0], size=B)
        r, d = z["buf_reward"][rows], z["buf_done"][rows]
    t = D.td_truth(q, z["learn/next_q"] if double else None, z["learn/next_target_q"] if double else z["learn/next_q"], a, r, d,
                   z["learn/weights"] if per else None, _h(z, "gamma"), _h(z, "alpha") if per else 0.0, n_step)
    return z, t, a


@pytest.mark.parametrize("name", ["dqn", "double", "multistep", "per", "ape_x"])
def test_td_truth_reproduces_the_reference_fixture(name):
    """Tolerances: those of _check_td / test_td_dqn_fixture (tests/test_kernels_gpu.py) for the same arrays."""
    z, t, a = _td_fixture(name)
    B = a.size
    np.testing.assert_allclose(t["loss"], z["learn/loss"], rtol=1e-5)
    np.testing.assert_allclose(t["max_Q"], z["result/max_Q"], rtol=1e-6)
    np.testing.assert_allclose(t["grad"][np.arange(B), a].reshape(B, 1), z["learn/d_q"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(t["y"].reshape(B, 1), z["learn/target_q"], rtol=1e-5, atol=1e-6)
    if name in ("per", "ape_x"):
        np.testing.assert_allclose(t["prio"].reshape(B, 1), z["learn/p_j"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(t["td"].reshape(B, 1), z["learn/td_error"], rtol=1e-5, atol=1e-6)
    else:
        np.testing.assert_allclose(t["prio"].reshape(B, 1), np.abs(z["learn/target_q"] - z["learn/q"]), atol=1e-6)
    if t["a_star"] is not None:
        assert np.array_equal(t["a_star"], z["learn/max_a"].reshape(B))
    other = np.ones(t["grad"].shape, bool)
    other[np.arange(B), a] = False
    assert not t["grad"][other].any()


# ----------------------------------------------------------------------------------------------- the three float32 supports
@pytest.mark.parametrize("v_min,v_max,K", [(-1, 10, 51), (-10, 10, 51), (-2, 3, 51), (-1, 10, 21), (-1, 10, 200)])
def test_default_support_is_torch_linspace_up_to_the_last_bit(v_min, v_max, K):
    """The truth's default support (the kernel's documented form, in numpy) against torch.linspace(v_min, v_max, K) on the CPU, element by
    element: at most 1 ulp apart (the ulp of the larger operand of the sum that forms the atom).  Atoms that differ from torch.linspace / from np.linspace(dtype=float32), as measured with the
    torch build this was written on:
        (-1, 10, 51): 9 / 13     (-10, 10, 51): 15 / 16     (-2, 3, 51): 16 / 17     (-1, 10, 21): 3 / 7     (-1, 10, 200): 36 / 43
    The first count is a property of torch's CPU path (its vectorised loop rounds step * k + v_min differently from the scalar symmetric
    form), not of the kernel, so it is printed and not asserted; expectations do not see it, floor / ceil of the projection do."""
    import torch

    ours = C.default_support(v_min, v_max, K)
    assert ours.dtype == np.float32 and ours[0] == np.float32(v_min) and ours[-1] == np.float32(v_max) and np.all(np.diff(ours) > 0)
    th = torch.linspace(v_min, v_max, K, dtype=torch.float32).numpy()
    lin = np.linspace(v_min, v_max, K, dtype=np.float32)
    k = np.arange(K)
    step = np.float32(np.float32(v_max) - np.float32(v_min)) / np.float32(K - 1)
    prod = np.abs(step * np.where(k < K // 2, k, K - 1 - k).astype(np.float32))
    # one ulp of the larger of the atom and the product step * k it was formed from (next to 0 an atom's own ulp is finer than the rounding
    # of the product that both forms add to v_min or take from v_max)
    ulp = np.spacing(np.maximum(np.abs(ours), prod).astype(np.float32)).astype(np.float64)
    d_th, d_np = np.abs(ours.astype(np.float64) - th) / ulp, np.abs(ours.astype(np.float64) - lin) / ulp
    print(f"support ({v_min}, {v_max}, {K}): {int((d_th > 0).sum())} atoms differ from torch.linspace (max {d_th.max():.2f} ulp), "
          f"{int((d_np > 0).sum())} from np.linspace (max {d_np.max():.2f} ulp)")
    assert d_th.max() <= 1.0, d_th


# ----------------------------------------------------------------------------------------------- the sweeps' conditions
def test_c51_sweep_covers_every_size_flag_and_variant():
    S = C.SWEEP
    assert len(set(S)) == len(S)
    assert {c[0] for c in S} == {1, 3, 63, 64, 65, 127, 128, 129, 200, 1024, 1025, 1027, 1030}
    assert {c[1] for c in S} == {1, 2, 3, 4, 5, 8, 9, 18}
    assert {c[2] for c in S} == {2, 51, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256}
    assert {c[3] for c in S} == {0, 1, 3, 64, 65}
    assert {c[4] for c in S} == set(C.FLAGS)
    assert {c[5] for c in S} == {"plain", "all_done", "terminal_first", "on_atoms", "outside", "clamped_p", "exact_tie", "action_clip"}
    for B in {c[0] for c in S if c[0] >= 129}:
        assert any(c[0] == B and "per" in c[4] for c in S), B
    assert any(c[0] <= 1024 and c[3] > 64 for c in S) and any(c[0] <= 1024 and c[3] == 64 for c in S)  # both sides of the block kernel's preload
    assert (3, 2, 192, 1) in {c[:4] for c in S} and C.BLOCK_VS_WAVE in S
    assert max(c[0] * c[1] * c[2] for c in S) * 4 * 3 < 8 << 20


@pytest.mark.parametrize("case", C.SWEEP, ids=[C.case_id(c) for c in C.SWEEP])
def test_c51_sweep_case_meets_the_conditions(case):
    B, A, K, n_step, flags, variant = case
    d, t, ro = c51_case(case)
    rows = np.arange(B)
    tie = t["gap"] == 0.0
    near = C.near_ties(t) & ~(tie if variant == "exact_tie" else False)
    counts = dict(near_ties=int(near.sum()), clamp=int((t["clamp_dist"] < 0.5).sum()), mass=int(((t["mass"] > 0) & (t["mass"] < 1e-6)).sum()),
                  l_u_differ=int((ro["l"] != t["l"]).any(-1).sum() + (ro["u"] != t["u"]).any(-1).sum()), a_star_differ=int((ro["target_action"].reshape(B) != t["a_star"]).sum()))
    print(f"{C.case_id(case)}: {counts}; rows with mass 0: {int((t['mass'] == 0).sum())}, exact ties: {int(tie.sum())}, terminal: {int(d['done'][:, 0].sum())}")
    assert counts == dict(near_ties=0, clamp=0, mass=0, l_u_differ=0, a_star_differ=0)
    assert np.isfinite(t["grad"]).all() and np.isfinite(t["kl"]).all() and (t["kl"] >= 0).all()
    act = np.clip(d["action"].astype(np.int64), 0, A - 1)
    p_act = t["p_act"]
    on_atom = (t["l"] == t["u"]) & (t["l"] > 0) & (t["l"] < K - 1)
    if variant != "exact_tie":
        assert int(tie.sum()) == 0
    if variant == "outside":
        assert int((t["mass"] == 0).sum()) >= 1 and np.abs(d["reward"]).max() == 20.0
    elif variant == "clamped_p":
        assert (p_act < C.FLOOR).any() and (p_act > C.FLOOR).any() and ((p_act < C.FLOOR).any(-1) & (t["mass"] > 0)).any()
    elif variant == "terminal_first":
        assert int(d["done"][:, 0].sum()) >= 1 and (n_step <= 1 or int((d["done"][:, 0] * (1 - d["done"][:, 1:]).max(-1)).sum()) >= 1)
    elif variant == "all_done":
        assert d["done"].all()
    elif variant == "on_atoms":
        assert on_atom.any() and (on_atom.all(-1) & (d["done"][:, 0] == 1)).any()
        assert n_step <= 1 or (on_atom.all(-1) & (d["done"][:, 0] == 0) & (t["mass"] == 0)).any()
    elif variant == "exact_tie":
        zn = d["next_online"]
        assert int(tie.sum()) >= 1
        for b in np.nonzero(tie)[0]:
            same = [a for a in range(A) if np.array_equal(zn[b, a], zn[b, t["a_star"][b]])]
            assert len(same) == 2 and t["a_star"][b] == min(same)
    elif variant == "action_clip":
        assert (d["action"] < 0).any() and (d["action"] > A - 1).any()
    assert not t["grad"][t["mass"] == 0].any()


def test_the_oracle_on_its_own_support_moves_an_atom_of_the_projection():
    """Why the oracle gets the truth's support: at (B, A, K, n) = (3, 2, 192, 1) its own np.linspace support puts at least one atom's l / u one
    atom away from the kernel's form, although the two supports are one ulp of v_max apart at the most."""
    case = next(c for c in C.SWEEP if c[:4] == (3, 2, 192, 1))
    d, t, ro = c51_case(case)
    B, A, K = d["logit"].shape
    own = O.c51_project_kl(d["logit"], np.clip(d["action"].astype(np.int64), 0, A - 1), d["reward"].reshape(B, -1, 1), d["done"].reshape(B, -1, 1), d["target"],
                           C.V_MIN, C.V_MAX, K, C.GAMMA, next_logit_online=d["next_online"], weights=d["weights"], alpha=C.ALPHA)
    assert np.abs(np.linspace(C.V_MIN, C.V_MAX, K, dtype=np.float32).astype(np.float64) - t["support"]).max() <= np.spacing(np.float32(C.V_MAX))
    moved = int(((own["l"] != t["l"]) | (own["u"] != t["u"])).sum())
    scale = np.abs(t["grad"]).max()
    print(f"atoms whose l / u differ under np.linspace: {moved}; gradient moves by {np.abs(own['d_logit'] - t['grad']).max() / scale:.2e} of its maximum "
          f"(on the truth's support: {np.abs(ro['d_logit'] - t['grad']).max() / scale:.2e})")
    assert moved >= 1
    assert np.abs(ro["d_logit"] - t["grad"]).max() <= 1e-5 * scale


def test_td_sweep_covers_every_size_and_flag():
    S = D.SWEEP
    assert len(set(S)) == len(S)
    assert {c[0] for c in S} == {1, 255, 256, 257, 513}
    assert {c[1] for c in S} == {1, 2, 6, 18}
    assert {(c[2], c[3]) for c in S if c[4] == "plain"} == {(n, f) for n in (0, 1, 3) for f in D.FLAGS}
    assert {c[4] for c in S} == {"plain", "zero_td", "action_clip"}


@pytest.mark.parametrize("case", D.SWEEP, ids=[D.case_id(c) for c in D.SWEEP])
def test_td_sweep_case_meets_the_conditions(case):
    B, A, n_step, flags, variant = case
    d, t, ro = td_case(case)
    huber = "per" not in flags
    counts = dict(kink=int((t["kink_dist"] < 1e-4).sum()) if huber else 0, near_ties=int(D.near_ties(t, d["q_next_online"]).sum()))
    print(f"{D.case_id(case)}: {counts}; rows with td == 0: {int((t['td'] == 0).sum())}, |td| < 1: {int((t['td'] < 1).sum())}, > 1: {int((t['td'] > 1).sum())}")
    assert counts == dict(kink=0, near_ties=0)
    if d["q_next_online"] is not None:
        assert np.array_equal(np.argmax(d["q_next_online"], -1), t["a_star"])
    np.testing.assert_allclose(ro["target_q"].reshape(B), t["y"], rtol=1e-5, atol=1e-6)
    if variant == "zero_td":
        assert int((t["td"] == 0).sum()) >= 1 and int((ro["td_error"] == 0).sum()) == int((t["td"] == 0).sum())
    elif variant == "action_clip":
        assert (d["action"] < 0).any() and (d["action"] > A - 1).any()
    if B >= 255 and huber:
        assert (t["td"] < 1).any() and (t["td"] > 1).any()
