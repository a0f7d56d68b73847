"""CPU-only checks of what tests/test_acting_truth_gpu.py stands on (tests/acting_truth.py): the case table reaches every acting path the
collector can select, the scripted env is what its replay says it is, and the sharp policies are sharp."""
import numpy as np
import pytest
import torch

import acting_truth as AT

T = AT.T_STEPS

# name -> what the case was written to reach (derived by hand from jh_collect.hip / jh_persist.hip; dispatch() must agree)
PINNED = {
    "b": dict(persist=1, lookahead=1, split=1, rows=32, SP=12, NCH=8, PI=2, RT=2, G=3, reduced=1),
    "c-W2": dict(persist=1, split=1, SP=4, NCH=1, PI=1, RT=2, G=1, reduced=0),
    "c-W3": dict(persist=1, split=1, G=1),
    "c-W31": dict(persist=1, split=1, rows=31, PI=1, G=1),
    "d": dict(persist=1, split=0, rows=25, SP=12, NCH=2, PI=2, RT=2, G=3),
    "e": dict(persist=1, split=0, SP=8, NCH=2, PI=1, RT=1, G=4),
    "f": dict(persist=1, split=0, SP=12, NCH=4, PI=2, RT=2, G=3),
    "g": dict(persist=1, split=0, SP=16, NCH=8, PI=1, RT=1, G=4),
    "h": dict(persist=1, split=0, SP=4, NCH=1, PI=1, RT=1, G=3),
    "i-W10": dict(persist=1, lookahead=2, split=1, rows=30, G=1),
    "i-W5": dict(persist=1, lookahead=2, split=1, rows=15, SP=8),
    "i-W2": dict(persist=1, lookahead=2, split=1, rows=6, SP=16),
    "j": dict(persist=1, lookahead=2, split=1, rows=30, NCH=8),
    "k": dict(persist=1, split=0, PI=3, RT=2, reduced=0),
    "l": dict(persist=1, split=0, SP=16, NCH=1, PI=4, RT=2, G=1),
    "m": dict(persist=1, lookahead=2, split=0, rows=30, RT=2),
    "n-f": dict(persist=1, split=0, RT=2, reduced=1),
    "n-a": dict(persist=1, split=1, SP=8, NCH=1, reduced=1),
    "n-i": dict(persist=1, lookahead=2, split=1, reduced=1),
    "o": dict(persist=1, split=1, reduced=0),
    "p-b": dict(persist=0, path="fused"),
    "p-e": dict(persist=0, path="separate"),
    "p-g": dict(persist=0, path="separate"),
    "q-S17": dict(persist=0, path="fused"),
    "q-cont13": dict(persist=0, path="separate"),
    "q-disc13": dict(persist=0, path="separate"),
    "r": dict(persist=1, split=0, SP=8, NCH=2, PI=2, RT=2, G=2),
}


def test_case_table_reaches_every_acting_path():
    names = [c["name"] for c in AT.CASES]
    assert len(names) == len(set(names)) == 53
    d = {c["name"]: AT.dispatch(c) for c in AT.CASES}
    for name, want in PINNED.items():
        got = {k: d[name][k] for k in want}
        assert got == want, (name, got, want)
    for S in (2, 7, 11, 16):
        for H in (64, 128, 256, 512):
            x = d[f"a-S{S}-H{H}"]
            assert (x["persist"], x["split"], x["rows"], x["G"], x["PI"]) == (1, 1, 4, 2, 1), (S, H, x)
    for H in (32, 96):
        for W in (1, 16, 17, 33):
            assert d[f"q-H{H}-W{W}"]["persist"] == 0 and d[f"q-H{H}-W{W}"]["path"] == "fused"
    per = [x for x in d.values() if x["persist"]]
    have = lambda *keys: {tuple(x[k] for k in keys) for x in per}
    assert have("SP", "NCH") == {(sp, nch) for sp in (4, 8, 12, 16) for nch in (1, 2, 4, 8)}
    assert have("PI") == {(1,), (2,), (3,), (4,)}
    assert have("G") == {(1,), (2,), (3,), (4,)}
    assert have("RT") == {(1,), (2,)}
    assert have("split") == {(0,), (1,)}
    assert have("reduced", "lookahead") >= {(0, 1), (0, 2), (1, 1), (1, 2)}  # the device-side sum and the host's, each with look-ahead rows too
    assert have("lookahead", "split") >= {(2, 0), (2, 1)}
    assert {(x["SP"] > 8) for x in per if x["PI"] > 1} == {False, True}  # W1 in registers and in LDS, each under more than one poll instruction
    assert {(x["reduced"], x["RT"], x["split"]) for x in per} >= {(1, 2, 0), (1, 2, 1)}  # summed on the device: unsplit tiles and halves
    step = [(c, d[c["name"]]) for c in AT.CASES if not d[c["name"]]["persist"]]
    assert {x["path"] for _, x in step} == {"fused", "separate"}
    for path in ("fused", "separate"):
        assert {AT.n_out_of(c) <= 8 for c, x in step if x["path"] == path} == {path == "fused"}
    widths = {c["W"] for c, _ in step}
    assert {1, 16, 17, 32, 33} <= widths  # both sides of a 16-row tile and of the persistent kernel's 32 rows
    # a switch variant is its base case with switches: same shapes, same weights, same env
    for c in AT.CASES:
        b = AT.by_name(c["base"])
        assert all(c[k] == b[k] for k in ("kind", "W", "S", "A", "H", "cont")) and AT.case_seed(c) == AT.case_seed(b)
        assert set(c["env"]) <= set(AT.SWITCHES)
    assert [c["name"] for c in AT.CASES if c["sharp"]] == ["e-sharp", "i-sharp"]


SCRIPTED = [c for c in AT.CASES if c["kind"].startswith("scripted") and c["name"] == c["base"]]


def _actions(case, rng, T_):
    W, A = case["W"], case["A"]
    return np.tanh(rng.randn(W, T_, A)).astype(np.float32) if case["cont"] else rng.randint(0, A, size=(W, T_)).astype(np.int64)


@pytest.mark.parametrize("case", SCRIPTED, ids=lambda c: c["name"])
def test_scripted_env_replays_bit_for_bit_and_ends_where_scripted(case):
    W, S = case["W"], case["S"]
    env, model = AT.make_env(case), AT.make_model(case)
    rng = np.random.RandomState(3)
    seen = []
    for run in range(AT.N_RUNS):
        a = _actions(case, rng, T)
        st, ns, rw, dn = (np.empty((W, T, S), np.float32), np.empty((W, T, S), np.float32), np.empty((W, T), np.float32), np.empty((W, T), np.uint8))
        for t in range(T):
            env.obs(st[:, t])
            env.step(a[:, t], ns[:, t], rw[:, t], dn[:, t])
        m = model.replay(a)
        for ours, theirs, what in zip((st, ns, rw, dn.astype(bool)), m, ("state", "next_state", "reward", "done")):
            assert ours.dtype == theirs.dtype and np.array_equal(ours, theirs), (what, run)
        if run == 0:
            assert dn[:, 1].any() and dn[:, T - 1].any(), "no episode ends at t = 1 / t = T - 1"
            assert dn[0, 1] and dn[0, T - 1]  # row 0 does both: a one-row case has them too
        go = dn[:, :-1] == 0  # where the episode goes on, the next row starts where this one ended; where it ended, it does not
        assert np.array_equal(ns[:, :-1][go], st[:, 1:][go]) and (ns[:, :-1][~go] != st[:, 1:][~go]).any(axis=-1).all()
        seen.append(st)
    x = np.concatenate([s.reshape(-1) for s in seen])
    assert x.dtype == np.float32 and (x == 0).any() and (x > 0).any() and (x < 0).any()
    mag = np.abs(x[x != 0])
    assert 1e-3 <= mag.min() < 1e-2 and 4.0 < mag.max() <= 8.0, (mag.min(), mag.max())
    # other actions, another trajectory: the observation depends on what was done
    other = AT.make_model(case).replay(_actions(case, np.random.RandomState(4), T))
    assert not np.array_equal(other[0][:, 1:], seen[0][:, 1:])


@pytest.mark.parametrize("case", [c for c in SCRIPTED if c["kind"] == "scripted-fork"], ids=lambda c: c["name"])
def test_scripted_env_forked_copy_on_row_ranges_equals_the_original(case):
    """What the look-ahead does with the table: copy rows into a scratch env of another size, step a RANGE of it; the range's arrays hold
    the range's rows."""
    W, S = case["W"], case["S"]
    env = AT.make_env(case)
    rng = np.random.RandomState(5)
    nxt, rew, dn = np.empty((W, S), np.float32), np.empty(W, np.float32), np.empty(W, np.uint8)
    env.step(_actions(case, rng, 1)[:, 0], nxt, rew, dn)  # off the start state
    scratch = env.fork(2 * W)
    for i in range(W):
        scratch.copy_row(2 * i, env, i)
        scratch.copy_row(2 * i + 1, env, i)
    assert np.array_equal(scratch.obs(np.empty((2 * W, S), np.float32))[0::2], env.obs())
    act = np.tile(np.array([0, 1], np.int64), W)
    whole = AT.make_env(case)
    whole.rid, whole.ep, whole.t, whole.chk = scratch.rid.copy(), scratch.ep.copy(), scratch.t.copy(), scratch.chk.copy()  # (2 W rows of state in a W-row shell)
    whole.W = 2 * W
    ref = (np.empty((2 * W, S), np.float32), np.empty(2 * W, np.float32), np.empty(2 * W, np.uint8))
    whole.step(act, *ref)
    cut = 2 * ((W + 1) // 2)
    for r0, r1 in ((0, cut), (cut, 2 * W)):
        n = r1 - r0
        out = (np.empty((n, S), np.float32), np.empty(n, np.float32), np.empty(n, np.uint8))
        scratch.step(act[r0:r1], *out, r0, r1)
        for o, r in zip(out, ref):
            assert np.array_equal(o, r[r0:r1])
        assert np.array_equal(scratch.obs(np.empty((n, S), np.float32), r0, r1), whole.obs()[r0:r1])
    assert not hasattr(AT.make_env(AT.by_name("e")), "fork")  # a plain scripted env offers no copies: one timestep per exchange


@pytest.mark.parametrize("name", ["e-sharp", "i-sharp"])
def test_sharp_policies_are_point_masses_on_the_rows_the_rollout_visits(name):
    """The input condition of the GPU test's "stored action == float64 argmax": rolled greedily in float64, at least 90 % of the visited rows
    carry p_max >= 1 - 1e-9 (the GPU test recomputes the mask on the rows it stored and asserts the same share)."""
    case = AT.by_name(name)
    m64, m32 = AT.sharp(case)
    for a, b in zip(m64.parameters(), m32.parameters()):
        assert torch.equal(a, b.double())  # float32-representable
    plain64, _ = AT.policy(case)
    assert all(float(p.detach().abs().min()) > 0 for p in plain64.parameters() if p.dim() == 1), "a bias sits on zero"
    states, pm = AT.greedy_rollout(case, m64)
    share = float((pm >= AT.SHARP_P).mean())
    print(f"{name}: {share:.3f} of {pm.size} rows decided, smallest p_max {pm.min():.6f}")
    assert share >= AT.SHARP_ROWS, share
    _, pm_plain = AT.greedy_rollout(case, plain64)
    assert float((pm_plain >= AT.SHARP_P).mean()) == 0.0  # the unscaled policy samples
