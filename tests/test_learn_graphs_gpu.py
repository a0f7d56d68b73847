"""ops.LearnGraphs through real agents: the call-by-call schedule of eager runs, captures and replays of every agent that has a capture policy of
its own (TD3, DDPG and SAC assert theirs in test_td3_gpu.py / test_sac_gpu.py), and the fallback of a capture that raises."""
import numpy as np
import pytest
import torch

from oracle import synth
from tests.util import refuse_capture

pytestmark = pytest.mark.gpu


def _value_rows(seed, n, S, A):
    rs = np.random.RandomState(seed)
    return {"state": rs.rand(n, S), "next_state": rs.rand(n, S), "action": rs.randint(0, A, size=(n, 1)), "reward": rs.rand(n, 1), "done": rs.rand(n, 1) < 0.2}


def _value_agent(name, use_graph=True, **kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    agent = Agent(name, state_size=4, action_size=2, hidden_size=32, optim_config={"name": "adam", "lr": 1e-3}, buffer_size=64, batch_size=8, start_train_step=0,
                  run_step=1000, device="cuda", use_graph=use_graph, **kw)
    agent.memory.first_store = False
    agent.memory.store_soa(_value_rows(1, 32, 4, 2))
    return agent


def _mpo():
    import mpo_truth
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    agent = Agent("mpo", state_size=4, action_size=3, hidden_size=32, optim_config={"name": "adam", "lr": 1e-3}, buffer_size=64, batch_size=8, start_train_step=0,
                  n_epoch=1, n_step=4, run_step=1000, device="cuda")
    agent.memory.first_store = False
    agent.memory.store(mpo_truth.replay(3, 16, 4, 4, 3))
    return agent


def _rollout_agent(name, S, A, H, W, T, B):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    head = dict(head="cnn") if isinstance(S, tuple) else {}
    agent = Agent(name, state_size=list(S) if head else S, action_size=A, hidden_size=H, network="discrete_policy_value", optim_config={"name": "adam", "lr": 1e-3},
                  batch_size=B, n_step=T, n_epoch=2, num_workers=W, run_step=100000, device="cuda", **head)
    agent.memory.first_store = False
    return agent


def _rollout(agent, S, A, M, it):
    """One process() = one learn() on M fresh rows (drawn off np.random's global state, which decides PPO's form: see TOUCH)."""
    rs = np.random.RandomState(10 + it)
    trs = synth.ppo_image_rollout(rs, M, S, A) if isinstance(S, tuple) else synth.ppo_rollout(rs, M, S, A, False, clamp_every=0)
    agent.process({k: np.concatenate([t[k] for t in trs], 0) for k in ("state", "next_state", "reward", "done", "action")}, (it + 1) * agent.n_step)


# np.random is drawn from before learns 3 and 4: PPO / V-MPO find their pre-drawn index lists stale there and take the split form (two graphs around the
# host's shuffles) that learn 0, before anything was pre-drawn, warmed; every other learn is the one-graph form
TOUCH = (3, 4)
ONE, SPLIT = "('one', False)", "('split', False)"
PPO_TABLE = [[], [], [ONE], [ONE, SPLIT, "main"], [ONE, SPLIT, "main"], [ONE, SPLIT, "main"]]
SINGLE_TABLE = [False, True, True, True, True, True]

# what `sorted(map(str, agent._graphs))` (rollout agents) or `agent._graph is not None` (one-graph agents) gives after each of six learns, recorded on the
# commit before ops.LearnGraphs existed, when each agent carried its own copy of the policy
SCHEDULES = {
    "dqn": (lambda: _value_agent("dqn"), lambda a, it: a.learn(), SINGLE_TABLE),
    "rainbow": (lambda: _value_agent("rainbow", n_step=1, num_support=11, v_min=-2, v_max=5), lambda a, it: a.learn(), SINGLE_TABLE),
    "mpo": (_mpo, lambda a, it: a.learn(), SINGLE_TABLE),
    "ppo": (lambda: _rollout_agent("ppo", 4, 2, 32, 2, 8, 8), lambda a, it: _rollout(a, 4, 2, 16, it), PPO_TABLE),
    "vmpo": (lambda: _rollout_agent("vmpo", 4, 2, 32, 4, 16, 24), lambda a, it: _rollout(a, 4, 2, 64, it), PPO_TABLE),
    "ppo_cnn": (lambda: _rollout_agent("ppo", (4, 44, 52), 4, 64, 2, 16, 16), lambda a, it: _rollout(a, (4, 44, 52), 4, 32, it), [[], ["learn"], ["learn"], ["learn"], ["learn"], ["learn"]]),
}


def schedule(name):
    """-> what is captured after each of six learns."""
    make, learn, expected = SCHEDULES[name]
    agent = make()
    np.random.seed(7)
    seen = []
    for it in range(6):
        if it in TOUCH:
            np.random.random()
        learn(agent, it)
        seen.append(agent._graph is not None if expected is SINGLE_TABLE else sorted(map(str, agent._graphs)))
    torch.cuda.synchronize()
    return seen, agent


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_capture_schedule(name):
    seen, agent = schedule(name)
    print(f"{name}: {seen}")
    assert seen == SCHEDULES[name][2]
    assert agent._graph is not None and not agent._learn_graphs.failed


def test_failed_capture_falls_back_to_eager_dqn(monkeypatch, capsys):
    """Four learns whose capture raises == four learns of an agent that never captures, bit for bit; the agent says so once and stays eager."""
    from jorldy_amd import ops

    monkeypatch.setattr(ops, "graph_capture", refuse_capture)
    out = []
    for use_graph in (True, False):
        agent = _value_agent("dqn", use_graph=use_graph)
        np.random.seed(7)
        res = [agent.learn() for _ in range(4)]
        torch.cuda.synchronize()
        assert agent._graph is None and not agent._graphs and agent._learn_graphs.failed == use_graph
        out.append((res, agent._net.params.clone(), agent._net.m.clone(), agent._net.v.clone()))
    assert out[0][0] == out[1][0], "results"
    for a, b in zip(out[0][1:], out[1][1:]):
        assert torch.equal(a, b), "weights and Adam moments"
    printed = capsys.readouterr().out
    assert printed.count("running eagerly") == 1
    assert "[jorldy_amd] hipGraph capture of DQN.learn() failed (RuntimeError: capture refused); running eagerly" in printed
