#!/usr/bin/env python3
"""Measurement of the Munchausen-DQN agent (core/agent/m_dqn.py on libjorldy_hip) at two shapes:

  cartpole   config.m_dqn.cartpole: S 4, A 2, hidden 512, B 32, Adam 1e-4, alpha 0.9, tau 0.03, l_0 -1
  atari      the config.m_dqn.atari learner: (4, 84, 84) uint8 frames, A 6, hidden 512, B 32, cnn head

Per shape: learn() in ms and updates/s, and single-mode env steps/s with act() on the GPU every step (epsilon 0: every act() is the
network; one store + one learn() per step as DQN.process does).  In the same process, alternating with it, Agent("dqn") at the same
shapes: the same networks, buffer and optimizer, so the difference is the forwards (the target trunk over 2B rows and the online
trunk over B, instead of the other way round) and the loss kernel.  One JSON line at the end.

    python tools/bench_mdqn.py [--updates 300] [--steps 300] [--rounds 3] [--shapes cartpole,atari]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

SHAPES = {
    "cartpole": dict(state_size=4, action_size=2, head="mlp", optim_config={"name": "adam", "lr": 1e-4}),
    "atari": dict(state_size=(4, 84, 84), action_size=6, head="cnn", optim_config={"name": "adam", "lr": 1e-4}),
}
FILL = 2048


def make_agent(name, shape):
    from jorldy_amd.core.agent import Agent

    kw = dict(SHAPES[shape], hidden_size=512, network="discrete_q_network", gamma=0.99, buffer_size=4096, batch_size=32, start_train_step=0,
              target_update_period=500, run_step=1_000_000, epsilon_init=0.0, epsilon_min=0.0, device="cuda")
    if name == "m_dqn":
        kw.update(alpha=0.9, tau=0.03, l_0=-1)
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    S, A = kw["state_size"], kw["action_size"]
    draw = (lambda m: rng.randint(0, 256, size=(m,) + tuple(S), dtype=np.uint8)) if isinstance(S, tuple) else (lambda m: rng.randn(m, S).astype(np.float32))
    cols = {"state": draw(FILL), "action": rng.randint(0, A, size=(FILL, 1)), "reward": rng.choice([0.0, 1.0], size=(FILL, 1)).astype(np.float32),
            "next_state": draw(FILL), "done": rng.rand(FILL, 1) < 0.02}
    agent.memory.store_soa(cols)
    one = [{k: v[i : i + 1] for k, v in cols.items()} for i in range(8)]
    return agent, one


def time_learn(agent, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.learn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def time_steps(agent, one, n, step0):
    """act() on the GPU + store + learn() per env step (run_mode.py:68-91 without an env behind it)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        tr = dict(one[i % len(one)])
        tr.update(agent.act(tr["state"], True))
        agent.process([tr], step0 + i + 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations m_dqn / dqn; the median is reported")
    ap.add_argument("--shapes", default="cartpole,atari")
    args = ap.parse_args()
    out = {"tool": "tools/bench_mdqn.py", "updates": args.updates, "steps": args.steps, "rounds": args.rounds, "shapes": {}}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        for shape in args.shapes.split(","):
            agents = {name: make_agent(name, shape) for name in ("m_dqn", "dqn")}
            for agent, _ in agents.values():
                time_learn(agent, args.warmup)
            learn = {k: [] for k in agents}
            step = {k: [] for k in agents}
            step0 = 0
            for _ in range(args.rounds):
                for name, (agent, one) in agents.items():
                    learn[name].append(time_learn(agent, args.updates))
                for name, (agent, one) in agents.items():
                    step[name].append(time_steps(agent, one, args.steps, step0))
                step0 += args.steps
            res = {}
            for name, (agent, _) in agents.items():
                ms, st = float(np.median(learn[name])) * 1e3, float(np.median(step[name]))
                res[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "env_steps_per_s_single_mode": round(1.0 / st, 1),
                             "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "learn_in_hipgraph": agent._graph is not None}
            res["m_dqn_over_dqn_learn"] = round(res["m_dqn"]["learn_ms"] / res["dqn"]["learn_ms"], 3)
            out["shapes"][shape] = res
            del agents
    else:
        out["device"] = None
    line = json.dumps(out)
    assert len(line) < 6000
    print(line)


if __name__ == "__main__":
    main()
