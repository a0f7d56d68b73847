#!/usr/bin/env python3
"""Measurement of the SAC agent (core/agent/sac.py on libjorldy_hip) at config.sac.mujoco's shapes: S 11, A 3, H 512, B 256, dynamic alpha,
Adam 5e-4 / 1e-3 / 3e-4 -- with TD3 (tools/bench_td3.py's agent at ITS config: B 128) in the same process for scale.

learn() in ms and updates/s (SAC: every learn is a critic update, an actor update and the temperature step, one hipGraph; the two [B, A]
normal draws before the replay are part of it), and single-mode env steps/s with act() on the GPU every step (one store + one learn() +
the soft update per step, as process() does).  SAC and TD3 alternate; the median of the rounds is reported.  Reads nothing from the
reference.  One JSON line at the end.

    python tools/bench_sac.py [--updates 300] [--steps 300] [--rounds 3]
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

import bench_td3 as T

S, A, H, B, FILL = 11, 3, 512, 256, 4096
OPT = {"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}


def make_agent():
    from jorldy_amd.core.agent import Agent

    agent = Agent("sac", state_size=S, action_size=A, hidden_size=H, optim_config=OPT, use_dynamic_alpha=True, gamma=0.99, tau=5e-3, buffer_size=8192, batch_size=B,
                  start_train_step=0, run_step=1_000_000, device="cuda")
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    cols = {"state": rng.randn(FILL, S).astype(np.float32), "action": np.tanh(rng.randn(FILL, A)).astype(np.float32),
            "reward": rng.randn(FILL, 1).astype(np.float32), "next_state": rng.randn(FILL, S).astype(np.float32), "done": rng.rand(FILL, 1) < 0.02}
    agent.memory.store_soa(cols)
    return agent, [{k: v[i : i + 1] for k, v in cols.items()} for i in range(8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations sac / td3; the median is reported")
    args = ap.parse_args()
    out = {"tool": "tools/bench_sac.py", "shape": "config.sac.mujoco (S 11, A 3, H 512, B 256); td3: config.td3.mujoco (B 128)", "updates": args.updates,
           "steps": args.steps, "rounds": args.rounds}
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sac.py measures on the GPU: no device found")
    out["device"] = torch.cuda.get_device_name(0)
    torch.manual_seed(0)
    np.random.seed(0)
    agents = {"sac": make_agent(), "td3": T.make_agent("td3")}
    for agent, one in agents.values():
        T.time_learn(agent, args.warmup)
        T.time_steps(agent, one, args.warmup, 0)  # warms the variant process() replays (SAC: learn + soft update)
    learn, step = {k: [] for k in agents}, {k: [] for k in agents}
    step0 = args.warmup
    for _ in range(args.rounds):
        for name, (agent, one) in agents.items():
            learn[name].append(T.time_learn(agent, args.updates))
        for name, (agent, one) in agents.items():
            step[name].append(T.time_steps(agent, one, args.steps, step0))
        step0 += args.steps
    for name, (agent, _) in agents.items():
        ms, st = float(np.median(learn[name])) * 1e3, float(np.median(step[name]))
        out[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "env_steps_per_s_single_mode": round(1.0 / st, 1),
                     "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "hipgraphs": len(agent._graphs)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
