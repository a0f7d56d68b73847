"""The collector's exchanges with the persistent acting kernel in two independent halves (jh_collect.hip: run_loop_lookahead and
run_loop_split with c->split; jh_persist.hip: PersistArgs::rows_rt) against one exchange of all rows (JH_COLLECT_SPLIT=0).  A half is
the same rows through the same arithmetic under the same sampling keys, so everything is compared BIT FOR BIT: the five rollout
columns, the captured heads / values / next values, the envs' observations after the run and the losses of the learn() between runs."""
import functools
import os
import time

import numpy as np
import pytest
import torch

from tests.util import npy

pytestmark = pytest.mark.gpu

COLS = ("state", "action", "reward", "next_state", "done")


class _Env:
    """os.environ for the duration of a block (the collector reads its switches when it is created / per run)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _make_env(kind, W, S, A):
    from jorldy_amd import ops

    if kind == "cartpole":
        return ops.CartPoleVec(W, seed=4)
    if kind == "control":
        return ops.ControlVec(W, S, A, seed=4)
    from tests.test_agents_gpu import _PyCartPole  # the forkable Python CartPole behind the function table

    return _PyCartPole(W, seed=4, forkable=True)


def _rollouts(kind, W, T, H, runs=3, stalls=None, **env):
    """`runs` rollouts of T timesteps with a learn() between them -> per run the columns, the capture, the env's observations, the losses
    (and the wall time of the run); stalls: JH_COLLECT_TEST_STALL per run."""
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import NativeCollector

    cont = kind == "control"
    S, A = (11, 3) if cont else (4, 2)
    with _Env(**env):
        torch.manual_seed(5)
        np.random.seed(5)
        agent = Agent("ppo", state_size=S, action_size=A, hidden_size=H, network="continuous_policy_value" if cont else "discrete_policy_value", n_step=T,
                      batch_size=min(64, W * T), n_epoch=1, device="cuda", seed=3, lr_decay=False, num_workers=W)
        agent.memory.first_store = False
        e = _make_env(kind, W, S, A)
        col = NativeCollector(e, agent, W)
        out = []
        for it in range(runs):
            with _Env(JH_COLLECT_TEST_STALL=stalls[it] if stalls else None):
                t_run = time.perf_counter()
                col.run(T)
                torch.cuda.synchronize()
                t_run = time.perf_counter() - t_run
            M, st, store = W * T, agent._static, agent.memory._store
            rec = {k: npy(store.column(k)[:M]).copy() for k in COLS}
            if col.capture:
                rec.update(h0=npy(st["h0"]).copy(), value=npy(st["value"]).copy(), next_value=npy(st["next_value"]).copy())
            obs = np.zeros((W, S), np.float32)
            rec["obs"] = np.array(e.obs(obs) if kind == "python" else e.obs()).copy()
            r = agent.process(None, T * (it + 1))  # a learn() between the runs: the next run acts with updated weights
            rec["loss"] = np.array([r["actor_loss"], r["critic_loss"], r["entropy_loss"]])
            rec["seconds"] = t_run
            out.append(rec)
        col.terminate()
    return out


@functools.lru_cache(maxsize=None)
def _one_exchange(kind, W, T, H, lookahead=None, capture="1"):
    """The reference, computed once per shape and left unchanged: one exchange of all rows."""
    return _rollouts(kind, W, T, H, JH_COLLECT_SPLIT="0", JH_COLLECT_LOOKAHEAD=lookahead, JH_COLLECT_CAPTURE=capture)


def _assert_same(ref, got, what):
    assert len(ref) == len(got)
    for it, (a, b) in enumerate(zip(ref, got)):
        assert set(a) == set(b)
        for k in a:
            if k != "seconds":
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, "run", it, k)


@pytest.mark.parametrize("T", [3, 4, 64])
@pytest.mark.parametrize("W", [2, 5, 8, 10])
def test_lookahead_in_two_halves_equals_one_exchange(W, T):
    """Two timesteps per exchange, halves of ceil(W/2) and floor(W/2) envs: 1 + 1, the odd 3 + 2, config.ppo.cartpole's 4 + 4 and the
    largest that fits a row tile (15 rows); odd T (a final one-step exchange), even T, and T = 64, where episodes end inside
    looked-ahead successors."""
    ref = _one_exchange("cartpole", W, T, 64)
    got = _rollouts("cartpole", W, T, 64)
    if T == 64:
        assert any(o["done"].any() for o in ref), "no episode ended: the reset path was not exercised"
    assert all("h0" in o and "value" in o and "next_value" in o for o in got)
    _assert_same(ref, got, "lookahead halves")


def test_lookahead_in_two_halves_at_the_flagship_width():
    ref = _one_exchange("cartpole", 8, 16, 512)
    _assert_same(ref, _rollouts("cartpole", 8, 16, 512), "lookahead halves, hidden 512")


def test_lookahead_in_two_halves_equals_one_timestep_per_exchange():
    ref = _one_exchange("cartpole", 8, 64, 64)
    one = _rollouts("cartpole", 8, 64, 64, JH_COLLECT_SPLIT="0", JH_COLLECT_LOOKAHEAD="1")
    _assert_same(one, ref, "one exchange: two timesteps vs one")
    _assert_same(one, _rollouts("cartpole", 8, 64, 64), "lookahead halves vs one timestep per exchange")


def test_lookahead_in_two_halves_on_a_python_env_behind_the_function_table():
    """Only scratch envs are stepped on row ranges; the env itself is read once and then moved on row by row with copy_row."""
    ref = _one_exchange("python", 5, 9, 64)
    _assert_same(ref, _rollouts("python", 5, 9, 64), "python env, lookahead halves")
    _assert_same(_one_exchange("cartpole", 5, 9, 64), ref, "python env vs the built-in one")


@pytest.mark.parametrize("capture", ["1", "0"])
@pytest.mark.parametrize("T", [3, 16])
@pytest.mark.parametrize("kind,W", [("cartpole", 2), ("cartpole", 8), ("cartpole", 9), ("cartpole", 17), ("control", 4), ("control", 7)])
def test_one_timestep_halves_equal_one_exchange(kind, W, T, capture):
    """run_loop_split for 2 <= W <= 32: the discrete CartPole with JH_COLLECT_LOOKAHEAD=1 (17: 9 + 8 rows) and the continuous control env."""
    ref = _one_exchange(kind, W, T, 64, lookahead="1", capture=capture)
    got = _rollouts(kind, W, T, 64, JH_COLLECT_LOOKAHEAD="1", JH_COLLECT_CAPTURE=capture)
    assert all(("h0" in o) == (capture == "1") for o in got)
    _assert_same(ref, got, "one-timestep halves")


@pytest.mark.parametrize("stall", ["2,0", "2,1"])
def test_lookahead_halves_hand_over_when_the_kernel_gives_up(stall):
    """JH_COLLECT_TEST_STALL idles the host for 0.35 s in front of a half's read at timestep 2: the acting kernel's bounded poll runs out
    (~0.2 s) and it exits.  In front of half 0 both halves stand at the same timestep when the loss is noticed; in front of half 1, half 0
    has stored an exchange that half 1 still owes, which is finished with one acting launch per timestep.  The rollout completes,
    every worker's trajectory is continuous, the rollout (its five columns, the envs it leaves) equals the unstalled one bit for bit, and
    the next run is normal.  The heads and values captured after the hand-over come from the per-launch acting kernel, which adds in another
    order than the persistent one: those are compared within fp32 summation noise (1e-5 on O(1) values), so the learn() that follows and the
    third run are not comparable bit for bit; the run before the stall is."""
    W, T = 4, 6
    ref = _rollouts("cartpole", W, T, 64)
    got = _rollouts("cartpole", W, T, 64, stalls=(None, stall, None))
    print("seconds per run:", [o["seconds"] for o in got])
    assert 0.35 <= got[1]["seconds"] < 2.0 and got[2]["seconds"] < 0.2, [o["seconds"] for o in got]
    for o in got:
        st, nx, dn = (o[k].reshape(W, T, -1) for k in ("state", "next_state", "done"))
        on = dn[:, :-1, 0] == 0  # where the episode goes on, the next row starts where this one ended
        assert np.array_equal(nx[:, :-1][on], st[:, 1:][on])
        assert all(np.isfinite(o[k]).all() for k in ("h0", "value", "next_value", "loss"))
    _assert_same(ref[:1], got[:1], "before the stall")
    for k in COLS + ("obs",):
        assert np.array_equal(ref[1][k], got[1][k]), ("stalled run", k)
    for k in ("h0", "value", "next_value"):
        print(k, "max difference after the hand-over:", np.abs(ref[1][k] - got[1][k]).max())
        np.testing.assert_allclose(got[1][k], ref[1][k], rtol=0, atol=1e-5, err_msg=k)


def test_lookahead_halves_device_side_sum_is_bit_identical():
    """JH_PERSIST_REDUCE=1 on the look-ahead halves: the same additions in tile order by a workgroup of each row tile."""
    host = _rollouts("cartpole", 8, 16, 64, JH_PERSIST_REDUCE="0")
    _assert_same(host, _rollouts("cartpole", 8, 16, 64, JH_PERSIST_REDUCE="1"), "device-side sum")
    _assert_same(_one_exchange("cartpole", 8, 16, 64), host, "halves vs one exchange")
