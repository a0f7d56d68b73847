"""R2D2's batched recurrent actors (csrc/jh_r2d2_actors.hip, ops.R2D2ActorFeed, manager.BatchedRecurrentActors) against the project's own host
path: N independent R2D2.interact_callback state machines (core/agent/r2d2.py, numpy) fed the same transitions in float64, and single-row
R2D2.act() calls on the learner's weights."""
import numpy as np
import pytest
import torch

import margins
from r2d2_actors_truth import done_from_sets, host_rows, trace
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

N, H, TICKS = 3, 8, 40
# an episode end at every phase of a window: at its first tick, n_step + 1 back from an emission, inside the burn-in, on two actors in the
# same tick (5, 21), on consecutive ticks (5-6, 20-21, 23-24)
DONES = ({5, 6, 17, 30}, {5, 12, 23, 24, 35}, {9, 20, 21, 33})
# (seq_len, n_burn_in, n_step, store_period, zero_padding, S, A); S = 5 / A = 3 copy by scalars, S = 8 / A = 4 by float4
CASES = ((4, 1, 3, 2, True, 5, 3), (4, 1, 3, 2, False, 5, 3), (6, 2, 1, 1, True, 5, 3), (5, 0, 2, 7, True, 5, 3), (4, 1, 3, 2, True, 8, 4))
GAMMA, ETA = 0.99, 0.9
# The ring keeps q in float32.  Rounding the float64 q of these cases to float32 before the float64 host fold moves the host priority by at most
# 4.96e-7 (measured over all cases with host_rows(q_as=np.float32), host only, no kernel involved: |q| <= 10.4, half a float32 ulp there is
# 4.8e-7, and a priority adds the errors of two q values); the kernel is allowed twice the measured gap.
PRIORITY_TOL = 2 * 4.96e-7


@pytest.mark.parametrize("case", CASES, ids=[f"seq{c[0]}-burn{c[1]}-n{c[2]}-period{c[3]}-pad{int(c[4])}-S{c[5]}" for c in CASES])
def test_emitted_rows_and_priorities_are_the_host_interact_callbacks(case):
    """Per tick: as many rows as the host emits, in ascending actor order, every column equal bit for bit (copies and zero fills), the float64
    priority within PRIORITY_TOL of the host's float64 value from unrounded q.  Rows pile up behind those of earlier ticks and start again from
    row 0 every 16 ticks; at tick 25 the state moves into a fresh object (state / load_state), which carries on."""
    from jorldy_amd import ops

    seq, burn, n, period, pad, S, A = case
    L = seq + n
    tr = trace(seq * 100 + n, TICKS, N, S, A, H, done_from_sets(DONES, TICKS))
    truth = host_rows(case, tr, GAMMA, ETA)
    lens = [int((r["state"][0] != 0).any(-1).sum()) for out in truth for _, r in out]
    assert L in lens and (not pad or min(lens) < L), "the schedule yields a full window and, with padding, a short one"
    feed = ops.R2D2ActorFeed(N, S, A, H, seq, burn, n, period, pad, GAMMA, ETA, "cuda:0")
    rows, count = feed.rows(16 * N), torch.zeros(1, dtype=torch.int64, device="cuda")
    act_out = (torch.zeros(N, dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.float32, device="cuda"))
    worst, held = 0.0, 0
    for t in range(TICKS):
        if t == 25:
            saved = feed.state()
            feed = ops.R2D2ActorFeed(N, S, A, H, seq, burn, n, period, pad, GAMMA, ETA, "cuda:0")
            feed.load_state(saved)
        held = 0 if t % 16 == 0 else held
        # eps = 1 > u = 0: every actor takes the injected action
        feed.act(f32(tr["q"][t]), f32(tr["obs"][t]), f32(tr["h"][t]), f32(tr["c"][t]), act_out, eps=np.ones(N), u=np.zeros(N), rand_action=tr["action"][t])
        feed.emit(tr["reward"][t], tr["done"][t], rows, count, restart=t % 16 == 0)
        torch.cuda.synchronize()
        assert np.array_equal(npy(act_out[0]), tr["action"][t]) and np.array_equal(npy(act_out[1]), tr["q"][t][np.arange(N), tr["action"][t]].astype(np.float32))
        assert int(count.item()) == held + len(truth[t]), f"tick {t}: rows emitted"
        for r, (a, want) in enumerate(truth[t], held):
            for k in ops.R2D2ActorFeed.COLS[:-1]:
                got = npy(rows[k][r])
                assert got.shape == want[k].shape[1:] and np.array_equal(got.astype(np.float64), want[k][0].astype(np.float64)), f"tick {t} actor {a} {k}"
            worst = max(worst, abs(rows["priority"][r].item() - want["priority"].item()))
        held += len(truth[t])
    print(f"{case}: largest |priority - float64 host priority| = {worst:.3e} (allowed {PRIORITY_TOL:.1e})")
    margins.leq(worst, PRIORITY_TOL, f"{case} actor-side priority vs the float64 host value")


def _agent(**over):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    kw = dict(state_size=4, action_size=3, hidden_size=64, network="r2d2", head="mlp", optim_config={"name": "adam", "lr": 1e-3}, batch_size=8, n_step=3, seq_len=4,
              n_burn_in=1, zero_padding=True, buffer_size=64, start_train_step=0, run_step=1000, lr_decay=False, use_graph=False, epsilon=0.5, gamma=0.99, eta=0.9)
    kw.update(over)
    return Agent("r2d2", **kw)


def test_batched_acting_is_seventeen_single_row_acts(monkeypatch):
    """17 actors (one row past a 16-row tile of jh_lstm_step) for 6 ticks against single-row R2D2.act() on the same weights, one carried state per
    actor swapped into the agent; both paths take their epsilon draws from the same injected arrays.  Two actors finish at tick 3."""
    from jorldy_amd.manager.batched_actors import BatchedRecurrentActors

    Na, ticks, agent = 17, 6, _agent()
    S, A = 4, 3
    actors = BatchedRecurrentActors(agent, Na, epsilons=np.full(Na, 0.5))
    rs = np.random.RandomState(4)
    obs, u, ra = rs.randn(ticks, Na, S).astype(np.float32), rs.random_sample((ticks, Na)), rs.randint(0, A, size=(ticks, Na))
    now = [0, 0]  # tick, actor (None: the batched call)
    monkeypatch.setattr(np.random, "random", lambda size=None: u[now[0]] if now[1] is None else u[now[0], now[1]])
    monkeypatch.setattr(np.random, "randint", lambda lo, hi, size=None: ra[now[0]] if now[1] is None else ra[now[0], now[1]].reshape(1, 1))
    carried = [(None, None)] * Na
    for t in range(ticks):
        done = np.asarray([t == 3 and a in (2, 16) for a in range(Na)])
        actors.stream.synchronize()  # the previous tick's emit may have zeroed a finished actor's state
        h_in, c_in, _, _, onehot = (npy(v) for v in actors.feed.carried())
        now[:] = [t, None]
        got = actors.act(obs[t])["action"]
        assert got.shape == (Na, 1) and got.dtype == np.int64
        for a in range(Na):
            now[1] = a
            agent.hidden, agent.prev_action = carried[a]
            out = agent.act(obs[t, a][None])
            assert np.array_equal(out["action"], got[a][None]), f"tick {t} actor {a}"
            assert np.array_equal(out["prev_action_onehot"].astype(np.float32)[0], onehot[a]), f"tick {t} actor {a}: the one-hot fed"
            margins.leq(np.abs(out["hidden_h"][0, 0] - h_in[a]).max(), 1e-5, f"tick {t} actor {a} carried h")
            margins.leq(np.abs(out["hidden_c"][0, 0] - c_in[a]).max(), 1e-5, f"tick {t} actor {a} carried c")
            carried[a] = (None, None) if done[a] else (agent.hidden, agent.prev_action)
        if t == 4:
            assert not h_in[[2, 16]].any() and not c_in[[2, 16]].any() and not onehot[[2, 16]].any() and h_in[3].any(), "a finished actor starts from zeros"
        actors.push(np.zeros(Na), done)
    greedy = actors.act(obs[0], training=False)["action"]
    actors.stream.synchronize()
    assert np.array_equal(greedy[:, 0], npy(actors._q).argmax(-1)), "training=False is greedy for every actor"


def test_collected_rows_feed_learn_end_to_end():
    """30 ticks of 4 synthetic CartPole envs -> drain_into the agent's PER buffer -> learn() on the drained rows."""
    from jorldy_amd import ops
    from jorldy_amd.manager.batched_actors import BatchedRecurrentActors

    agent = _agent(action_size=2)
    env, actors = ops.CartPoleVec(4, seed=3), BatchedRecurrentActors(agent, 4)
    assert np.allclose(actors.eps, [0.5 ** (1 + i / 3 * agent.epsilon_alpha) for i in range(4)], rtol=1e-6), "Ape-X's epsilon schedule (ape_x.py:166-172)"
    np.random.seed(1)
    obs, total = env.obs(), 0
    for _ in range(30):
        action = actors.act(obs)["action"]
        total += actors.drain_into(agent.memory)  # the rows of the ticks before: their count came down with the actions
        obs, reward, done = env.step(action.reshape(-1))
        actors.push(reward, done)
    total += actors.drain_into(agent.memory)      # the last tick's: waits for its count
    assert total > 0 and agent.memory.size == total == actors.stored_rows
    res = agent.learn()
    assert np.isfinite(res["loss"]) and np.isfinite(res["sampled_p"]) and res["sampled_p"] > 0


def test_unsupported_sizes_and_agents_are_refused_before_any_launch():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager.batched_actors import BatchedRecurrentActors

    with pytest.raises(JhError, match="seq_len . n_step"):
        ops.R2D2ActorFeed(2, 4, 2, 8, 128, 1, 33, 64, True, 0.99, 0.9, "cuda:0")
    with pytest.raises(ValueError, match="seq_len . n_step"):
        BatchedRecurrentActors(_agent(seq_len=128, n_step=33), 2)
    with pytest.raises(ValueError, match="n_actors"):
        BatchedRecurrentActors(_agent(), 1025)
    with pytest.raises(JhError, match="n_actors"):
        ops.R2D2ActorFeed(1025, 4, 2, 8, 4, 1, 3, 2, True, 0.99, 0.9, "cuda:0")
    dqn = Agent("dqn", state_size=4, action_size=2, hidden_size=64, buffer_size=64, batch_size=8)
    with pytest.raises(ValueError, match="R2D2"):
        BatchedRecurrentActors(dqn, 2)
