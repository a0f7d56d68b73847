#!/usr/bin/env python3
"""Measurement of the NoisyNet agent (core/agent/noisy.py on libjorldy_hip, engine kind 4) at two shapes:

  cartpole   config.noisy.cartpole: S 4, A 2, hidden 512, B 32, Adam
  atari      the config.noisy.atari learner: (4, 84, 84) uint8 frames, A 6, hidden 512, B 32, cnn head

Per shape: learn() in ms (hipGraph replay, after warm-up, host clock around `--updates` calls that end in a device synchronise), in the
same process and alternating with it Agent("rainbow") and Agent("dqn") at the same shapes.  Noisy does a subset of Rainbow's work (two
forwards instead of three, two noisy layers instead of four, the TD loss instead of C51 with PER), so the expectation is noisy <= rainbow.
Also the number of library launches of one learn() body (= the kernels of its captured graph), counted on an eager run under the library's
launch profile.  One JSON line at the end.

    python tools/bench_noisy.py [--updates 300] [--rounds 3] [--shapes cartpole,atari]
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
NAMES = ("noisy", "rainbow", "dqn")


def make_agent(name, shape, use_graph=True):
    from jorldy_amd.core.agent import Agent

    kw = dict(SHAPES[shape], hidden_size=512, gamma=0.99, buffer_size=4096, batch_size=32, start_train_step=0, target_update_period=500, run_step=1_000_000,
              device="cuda", use_graph=use_graph)
    if name == "rainbow":
        kw.update(n_step=4)  # config.rainbow's
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    S, A = kw["state_size"], kw["action_size"]
    draw = (lambda m: rng.randint(0, 256, size=(m,) + tuple(S), dtype=np.uint8)) if isinstance(S, tuple) else (lambda m: rng.randn(m, S).astype(np.float32))
    shape_r = (FILL, 4, 1) if name == "rainbow" else (FILL, 1)  # Rainbow stores n-step columns
    cols = {"state": draw(FILL), "action": rng.randint(0, A, size=(FILL, 1)), "reward": rng.choice([0.0, 1.0], size=shape_r).astype(np.float32),
            "next_state": draw(FILL), "done": rng.rand(*shape_r) < 0.02}
    agent.memory.store_soa(cols)
    return agent


def time_learn(agent, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.learn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def launches_per_learn(name, shape):
    """Library launches of one learn() body: an eager agent under the launch profile (which keeps learn() out of its graph)."""
    from jorldy_amd import ops

    agent = make_agent(name, shape, use_graph=False)
    agent.learn()
    ops.lib_profile(True)
    agent.learn()
    rep = ops.lib_profile_report()
    ops.lib_profile(False)
    return {k: v[0] for k, v in sorted(rep.items()) if not k.startswith("__")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations noisy / rainbow / dqn; the median is reported")
    ap.add_argument("--shapes", default="cartpole,atari")
    args = ap.parse_args()
    out = {"tool": "tools/bench_noisy.py", "updates": args.updates, "rounds": args.rounds, "shapes": {}}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        for shape in args.shapes.split(","):
            agents = {name: make_agent(name, shape) for name in NAMES}
            for agent in agents.values():
                time_learn(agent, args.warmup)
            learn = {k: [] for k in agents}
            for _ in range(args.rounds):
                for name, agent in agents.items():
                    learn[name].append(time_learn(agent, args.updates))
            res = {}
            for name, agent in agents.items():
                ms = float(np.median(learn[name])) * 1e3
                res[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]],
                             "learn_in_hipgraph": agent._graph is not None}
            res["noisy_over_rainbow_learn"] = round(res["noisy"]["learn_ms"] / res["rainbow"]["learn_ms"], 3)
            res["noisy_over_dqn_learn"] = round(res["noisy"]["learn_ms"] / res["dqn"]["learn_ms"], 3)
            del agents
            per = launches_per_learn("noisy", shape)
            res["noisy_launches_per_learn"] = sum(per.values())
            res["noisy_launches"] = per
            out["shapes"][shape] = res
    else:
        out["device"] = None
    print(json.dumps(out))


if __name__ == "__main__":
    main()
