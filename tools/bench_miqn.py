#!/usr/bin/env python3
"""Measurement of the M-IQN agent (core/agent/m_iqn.py on libjorldy_hip) at config.m_iqn.cartpole shapes: S 4, A 2, width 512, B 32,
N 64 samples, E 64 cosine features, Adam 1e-4 eps 1e-2/32, alpha 0.9, tau 0.03, l_0 -1 -- 2 048 network rows per forward, 6 144 per
learn(), as IQN's.

learn() in ms and updates/s, and single-mode env steps/s with act() on the GPU every step (epsilon 0: every act() is the network +
jh_iqn_act; one store + one learn() per step as DQN.process does).  In the same process, alternating with it, Agent("iqn") at
config.iqn.cartpole shapes: the same network and row count under the greedy target.  Reads nothing from the reference.  One JSON line
at the end.

    python tools/bench_miqn.py [--updates 300] [--steps 300] [--rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from bench_iqn import FILL, time_learn, time_steps  # noqa: E402


def make_agent(name):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=4, action_size=2, optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}, gamma=0.99, buffer_size=4096, batch_size=32,
              start_train_step=0, target_update_period=500, run_step=1_000_000, epsilon_init=0.0, epsilon_min=0.0, num_sample=64, embedding_dim=64, device="cuda")
    if name == "m_iqn":
        kw.update(alpha=0.9, tau=0.03, l_0=-1)
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    cols = {"state": rng.randn(FILL, 4).astype(np.float32), "action": rng.randint(0, 2, size=(FILL, 1)), "reward": rng.choice([0.0, 1.0], size=(FILL, 1)).astype(np.float32),
            "next_state": rng.randn(FILL, 4).astype(np.float32), "done": rng.rand(FILL, 1) < 0.02}
    agent.memory.store_soa(cols)
    return agent, [{k: v[i : i + 1] for k, v in cols.items()} for i in range(8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations m_iqn / iqn; the median is reported")
    args = ap.parse_args()
    out = {"tool": "tools/bench_miqn.py", "shape": "config.m_iqn.cartpole", "updates": args.updates, "steps": args.steps, "rounds": args.rounds}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        agents = {name: make_agent(name) for name in ("m_iqn", "iqn")}
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
        for name, (agent, _) in agents.items():
            ms, st = float(np.median(learn[name])) * 1e3, float(np.median(step[name]))
            out[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "env_steps_per_s_single_mode": round(1.0 / st, 1),
                         "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "learn_in_hipgraph": agent._graph is not None,
                         "rows_per_forward": int(32 * agent._net.K)}
        out["m_iqn_over_iqn_learn"] = round(out["m_iqn"]["learn_ms"] / out["iqn"]["learn_ms"], 3)
    else:
        out["device"] = None
    line = json.dumps(out)
    assert len(line) < 6000
    print(line)


if __name__ == "__main__":
    main()
