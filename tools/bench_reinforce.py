#!/usr/bin/env python3
"""Measurement of the REINFORCE agent (core/agent/reinforce.py on libjorldy_hip) at config.reinforce.cartpole's shapes: S 4, A 2 discrete,
hidden 512, Adam 1e-4, gamma 0.99, standardised returns.

  learn()        in ms at episodes of T = 32, 200 and 500 rows: the rows are uploaded first (untimed), then learn() -- sample, forward, the return
                 scan, the loss, backward, Adam, the loss read back -- between two host clock readings that both follow a device synchronise.
                 learn() is eager (T changes with every episode: no hipGraph).  The three lengths alternate; the median of the rounds is reported.
  launches       the library's kernel launches of one learn at each T, counted by its own per-kernel timers: they must be equal at all three
  single loop    env steps per second of the single-mode loop (act, env step, process) on the native CartPole, over --steps steps
  ppo            in the same process, alternating with the above: PPO's learn() at config.ppo.cartpole's shapes (1 worker x 128 steps,
                 minibatches of 32, 3 epochs) through process() of an uploaded rollout

Reads nothing from the reference.  One JSON line.

    python tools/bench_reinforce.py [--iters 1000] [--rounds 3] [--steps 5000]
    python tools/bench_reinforce.py --curve [--seeds 1,2,3]    the curve of tests/golden/curves_reference_reinforce.json's configuration
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

S, A, H = 4, 2, 512
LENGTHS = (32, 200, 500)
CONFIG = dict(state_size=S, action_size=A, hidden_size=H, network="discrete_policy", head="mlp", optim_config={"name": "adam", "lr": 1e-4}, gamma=0.99,
              use_standardization=True, lr_decay=True)


def make_agent(run_step=100000, **over):
    from jorldy_amd.core.agent import Agent

    kw = dict(CONFIG, run_step=run_step, device="cuda")
    kw.update(over)
    agent = Agent("reinforce", **kw)
    agent.memory.first_store = False
    return agent


def episode(rows):
    rng = np.random.RandomState(rows)
    reward = np.full((rows, 1), 0.1)
    reward[-1] = -1.0
    done = np.zeros((rows, 1), bool)
    done[-1] = True
    return {"state": rng.randn(rows, S).astype(np.float32), "action": rng.randint(0, A, size=(rows, 1)), "reward": reward,
            "next_state": rng.randn(rows, S).astype(np.float32), "done": done}


def time_learn(agent, cols, n):
    """-> seconds per learn(); the upload of the rows is outside the timed window."""
    total = 0.0
    for _ in range(n):
        agent.memory.store_soa(cols)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.learn()
        torch.cuda.synchronize()
        total += time.perf_counter() - t0
    return total / n


def launches(agent, cols):
    """One learn with the library's per-kernel timers on -> ({kernel: launches}, total)."""
    from jorldy_amd import ops

    agent.memory.store_soa(cols)
    torch.cuda.synchronize()
    ops.lib_profile(True)
    agent.learn()
    torch.cuda.synchronize()
    per = {k: v[0] for k, v in ops.lib_profile_report().items()}
    ops.lib_profile(False)
    return per, sum(per.values())


class PPOLeg:
    """PPO at config.ppo.cartpole's shapes: process() of an uploaded rollout = one learn()."""

    def __init__(self):
        from jorldy_amd.core.agent import Agent

        self.T = 128
        self.agent = Agent("ppo", state_size=S, action_size=A, hidden_size=H, network="discrete_policy_value", optim_config={"name": "adam", "lr": 2.5e-4}, gamma=0.99,
                           batch_size=32, n_step=self.T, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, clip_grad_norm=1.0, lr_decay=True,
                           run_step=1_000_000_000, num_workers=1, device="cuda")
        self.agent.memory.first_store = False
        self.cols, self.step = episode(self.T), 0
        self.cols["done"][-1] = False

    def run(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step += self.T
            self.agent.process(self.cols, self.step)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n


def single_loop(steps, seed, config=None, run_step=None, chunk=1000):
    """run_mode.py's single loop on the native CartPole (act, env step, process([transition], step)) -> (mean episode length per `chunk` env
    steps, env steps per second, episodes learnt from)."""
    from jorldy_amd.ops import CartPoleVec

    torch.manual_seed(seed)
    np.random.seed(seed)
    agent = make_agent(run_step or steps, **(config or {}))
    env = CartPoleVec(1, seed=1000 + seed)
    out, lens, ep = [], [], 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(1, steps + 1):
        state = env.obs().copy()
        a = agent.act(state, True)
        nxt, rew, done = env.step(a["action"].reshape(-1))
        tr = {"state": state, "next_state": np.array(nxt, np.float32), "reward": np.asarray(rew, np.float64).reshape(1, 1), "done": np.asarray(done).reshape(1, 1).astype(bool)}
        tr.update(a)
        agent.process([tr], step)
        ep += 1
        if bool(np.asarray(done).reshape(-1)[0]):
            lens.append(ep)
            ep = 0
        if step % chunk == 0:
            out.append(round(float(np.mean(lens)) if lens else float(ep), 1))
            lens = []
    torch.cuda.synchronize()
    return out, steps / (time.perf_counter() - t0), agent._adam_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3, help="alternations over the episode lengths and PPO; the median is reported")
    ap.add_argument("--steps", type=int, default=5000, help="env steps of the single-loop measurement")
    ap.add_argument("--curve", action="store_true")
    ap.add_argument("--seeds", default="1,2,3")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_reinforce.py measures on the GPU: no device found")
    out = {"tool": "tools/bench_reinforce.py", "device": torch.cuda.get_device_name(0)}
    if args.curve:
        import reinforce_truth as D

        c = D.CURVE_CONFIG
        curves = {s: single_loop(c["steps"], int(s), config=c["agent"], run_step=c["run_step"], chunk=c["chunk"])[0] for s in args.seeds.split(",")}
        tenths = {s: D.curve_tenths(v) for s, v in curves.items()}
        out["curve"] = {"config": c, "metric": f"mean episode length per {c['chunk']} env steps", "episode_length": curves,
                        "first_last_tenths": {s: [round(t[0], 1), round(t[1], 1)] for s, t in tenths.items()}}
        print(json.dumps(out))
        return
    torch.manual_seed(0)
    np.random.seed(0)
    agent, ppo = make_agent(), PPOLeg()
    cols = {T: episode(T) for T in LENGTHS}
    for T in LENGTHS:
        time_learn(agent, cols[T], args.warmup)
    ppo.run(args.warmup)
    times, ppo_times = {T: [] for T in LENGTHS}, []
    for _ in range(args.rounds):
        for T in LENGTHS:
            times[T].append(time_learn(agent, cols[T], args.iters))
        ppo_times.append(ppo.run(max(1, args.iters // 4)))
    counts = {T: launches(agent, cols[T]) for T in LENGTHS}
    out.update(shape=f"config.reinforce.cartpole: S {S}, A {A} discrete, H {H}", iters=args.iters, rounds=args.rounds,
               learn_ms={str(T): round(float(np.median(times[T])) * 1e3, 4) for T in LENGTHS},
               learn_ms_rounds={str(T): [round(v * 1e3, 4) for v in times[T]] for T in LENGTHS},
               launches_per_learn={str(T): counts[T][1] for T in LENGTHS}, launches_equal=len({counts[T][1] for T in LENGTHS}) == 1,
               launches_of_one_learn=counts[LENGTHS[0]][0], learn_in_hipgraph=agent._graph is not None,
               ppo_learn_ms=round(float(np.median(ppo_times)) * 1e3, 4), ppo_learn_ms_rounds=[round(v * 1e3, 4) for v in ppo_times],
               ppo_shape="config.ppo.cartpole: 1 x 128 rows, minibatches of 32, 3 epochs (12 updates)")
    curve, rate, learns = single_loop(args.steps, 1)
    out["single_loop"] = {"steps": args.steps, "env_steps_per_s": round(rate, 1), "learns": learns, "episode_length": curve}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
