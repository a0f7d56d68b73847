#!/usr/bin/env python3
"""Measurement of the R2D2 agent (core/agent/r2d2.py on libjorldy_hip) at two shapes:

  cartpole   config.r2d2.cartpole: S 4, A 2, hidden 512, B 64, seq_len 4, n_burn_in 1, n_step 3, Adam 1e-4, clip 40
  default    the class defaults at the same observation: seq_len 80, n_burn_in 40, n_step 4

Per shape: learn() in ms (the hipGraph replay, statistics read back each time), the library's kernel launches of one learn (counted by its own
per-kernel timers over one eager learn) and how the time of that eager learn splits between the LSTM step launches (forward and backward)
and everything else (the batched GEMMs, the loss, clip + Adam).  In the same process, alternating with it, Agent("ape_x") -- R2D2's parent
class: one transition per row, a q-network without memory -- at the same observation, hidden size and batch.  One JSON line.

    python tools/bench_r2d2.py [--updates 200] [--rounds 3] [--shapes cartpole,default]
    python tools/bench_r2d2.py --curve [--steps 12000] [--seeds 1,2,3]    the single-mode CartPole loop: mean episode length per 1000 env steps
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

SHAPES = {"cartpole": dict(seq_len=4, n_burn_in=1, n_step=3), "default": dict(seq_len=80, n_burn_in=40, n_step=4)}
S, A, H, B, FILL = 4, 2, 512, 64, 512


def make_agent(name, shape):
    from jorldy_amd.core.agent import Agent

    rng = np.random.RandomState(0)
    kw = dict(state_size=S, action_size=A, hidden_size=H, head="mlp", optim_config={"name": "adam", "lr": 1e-4}, gamma=0.99, buffer_size=1024, batch_size=B,
              start_train_step=0, clip_grad_norm=40.0, alpha=0.6, beta=0.6, run_step=1_000_000, device="cuda")
    if name == "r2d2":
        kw.update(SHAPES[shape], network="r2d2")
        L = kw["seq_len"] + kw["n_step"]
        act = rng.randint(0, A, size=(FILL, L))
        cols = {"hidden_h": (0.1 * rng.randn(FILL, 1, H)).astype(np.float32), "hidden_c": (0.1 * rng.randn(FILL, 1, H)).astype(np.float32),
                "next_hidden_h": (0.1 * rng.randn(FILL, 1, H)).astype(np.float32), "next_hidden_c": (0.1 * rng.randn(FILL, 1, H)).astype(np.float32),
                "state": rng.randn(FILL, L, S).astype(np.float32), "reward": rng.choice([0.1, -1.0], size=(FILL, L - 1, 1)).astype(np.float32),
                "done": rng.rand(FILL, L - 1, 1) < 0.02, "action": act[:, 1:, None], "prev_action_onehot": np.eye(A, dtype=np.float32)[act]}
    else:
        kw.update(network="discrete_q_network", n_step=SHAPES[shape]["n_step"])
        n = kw["n_step"]
        cols = {"state": rng.randn(FILL, S).astype(np.float32), "action": rng.randint(0, A, size=(FILL, 1)), "reward": rng.choice([0.1, -1.0], size=(FILL, n, 1)).astype(np.float32),
                "next_state": rng.randn(FILL, S).astype(np.float32), "done": rng.rand(FILL, n, 1) < 0.02}
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    agent.memory.store_soa(cols, priorities=rng.uniform(0.1, 1.0, size=FILL))
    return agent


def time_learn(agent, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.learn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def launches(agent):
    """One learn with the library's per-kernel timers on (it runs eagerly) -> ({kernel: (launches, ms)}, total launches)."""
    from jorldy_amd import ops

    ops.lib_profile(True)
    agent.learn()
    torch.cuda.synchronize()
    per = {k: (v[0], v[1]) for k, v in ops.lib_profile_report().items()}
    ops.lib_profile(False)
    return per, sum(v[0] for v in per.values())


def curve(steps, seed, chunk=1000):
    """run_mode.py's single loop on the native CartPole: act -> env -> interact_callback -> process when a row was emitted; config.r2d2.cartpole with
    run_step = steps -> mean episode length per `chunk` env steps: the metric and the loop of tests/golden/curves_reference_r2d2.json."""
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.ops import CartPoleVec

    torch.manual_seed(seed)
    np.random.seed(seed)
    agent = Agent("r2d2", state_size=4, action_size=2, hidden_size=512, network="r2d2", head="mlp", optim_config={"name": "adam", "lr": 1e-4}, gamma=0.99,
                  buffer_size=50000, batch_size=64, clip_grad_norm=40.0, start_train_step=2000, target_update_period=500, lr_decay=True, n_step=3, alpha=0.6,
                  beta=0.6, uniform_sample_prob=1e-3, seq_len=4, n_burn_in=1, zero_padding=True, run_step=steps, device="cuda")
    agent.memory.first_store = False
    env = CartPoleVec(1, seed=1000 + seed)
    state, out, lens, ep = env.obs(), [], [], 0
    for step in range(1, steps + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(a["action"].reshape(-1))
        tr = {"state": state, "next_state": nxt, "reward": np.asarray(rew, np.float64).reshape(1, 1), "done": np.asarray(done).astype(bool).reshape(1, 1)}
        tr.update(a)
        row = agent.interact_callback(tr)
        if row:  # run_mode.py:78-80: process() runs only when a row was emitted
            agent.process([row], step)
        state = env.obs()
        ep += 1
        if bool(np.asarray(done).reshape(-1)[0]):
            lens.append(ep)
            ep = 0
        if step % chunk == 0:
            out.append(round(float(np.mean(lens)) if lens else float(ep), 1))
            lens = []
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="alternations r2d2 / ape_x; the median is reported")
    ap.add_argument("--shapes", default="cartpole,default")
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--steps", type=int, default=12000)
    ap.add_argument("--seeds", default="1,2,3")
    args = ap.parse_args()
    out = {"tool": "tools/bench_r2d2.py", "updates": args.updates, "rounds": args.rounds, "device": None}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        if args.curve:
            curves = {s: curve(args.steps, int(s)) for s in args.seeds.split(",")}
            start, end = float(np.mean([np.mean(c[:2]) for c in curves.values()])), float(np.mean([np.mean(c[-4:]) for c in curves.values()]))
            out["curve"] = {"steps": args.steps, "metric": "mean episode length per 1000 env steps", "episode_length": curves, "start": round(start, 1), "end": round(end, 1),
                            "learns": bool(start < 40 and end > 4 * start)}  # the criteria tools/gen_golden_r2d2.py applies to the reference's curve
        else:
            out["shapes"] = {}
            for shape in args.shapes.split(","):
                torch.manual_seed(0)
                np.random.seed(0)
                agents = {name: make_agent(name, shape) for name in ("r2d2", "ape_x")}
                for agent in agents.values():
                    time_learn(agent, args.warmup)
                learn = {k: [] for k in agents}
                for _ in range(args.rounds):
                    for name, agent in agents.items():
                        learn[name].append(time_learn(agent, args.updates))
                res = {}
                for name, agent in agents.items():
                    per, total = launches(agent)
                    res[name] = {"learn_ms": round(float(np.median(learn[name])) * 1e3, 4), "launches_per_learn": total,
                                 "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "learn_in_hipgraph": agent._graph is not None}
                    if name == "r2d2":
                        step = {k: v for k, v in per.items() if "lstm_step" in k}
                        res[name].update(SHAPES[shape], step_launches=sum(v[0] for v in step.values()), eager_step_ms=round(sum(v[1] for v in step.values()), 4),
                                         eager_other_ms=round(sum(v[1] for k, v in per.items() if k not in step), 4), launches_of_one_learn={k: v[0] for k, v in per.items()})
                res["r2d2_over_ape_x_learn"] = round(res["r2d2"]["learn_ms"] / res["ape_x"]["learn_ms"], 3)
                out["shapes"][shape] = res
                del agents
    print(json.dumps(out))


if __name__ == "__main__":
    main()
