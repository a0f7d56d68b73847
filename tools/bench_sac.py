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


def make_discrete_agent():
    """The discrete SAC at config.sac.cartpole_discrete's shapes (S 4, A 2, H 512, B 64, dynamic alpha, Adam 1.5e-4 / 3e-4 / 1e-5)."""
    from jorldy_amd.core.agent import Agent

    agent = Agent("sac", state_size=4, action_size=2, hidden_size=512, actor="discrete_policy", critic="discrete_q_network", use_dynamic_alpha=True, gamma=0.99,
                  optim_config=dict(OPT, actor_lr=1.5e-4, critic_lr=3e-4, alpha_lr=1e-5), buffer_size=8192, batch_size=64, start_train_step=0, target_update_period=500,
                  run_step=1_000_000, device="cuda")
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    agent.memory.store_soa({"state": rng.randn(FILL, 4).astype(np.float32), "action": rng.randint(0, 2, size=(FILL, 1)), "reward": rng.randn(FILL, 1).astype(np.float32),
                            "next_state": rng.randn(FILL, 4).astype(np.float32), "done": rng.rand(FILL, 1) < 0.02})
    return agent


def discrete_curve(seed, c):
    """The discrete SAC in the single-mode loop (act, step, process([transition], step)) on ops.CartPoleVec at the configuration `c` of
    tests/golden/curves_reference_sac_discrete.json -> mean episode length per c["chunk"] env steps (--discrete --curve; tests/test_sac_discrete_gpu.py)."""
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    np.random.seed(seed)
    torch.manual_seed(seed)
    t = c["sac"]
    agent = Agent("sac", device="cuda", state_size=4, action_size=2, hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"],
                  run_step=c["run_step"], gamma=c["gamma"], lr_decay=c["lr_decay"], target_update_period=c["target_update_period"], actor="discrete_policy",
                  critic="discrete_q_network", use_dynamic_alpha=t["use_dynamic_alpha"], optim_config=dict(OPT, actor_lr=t["actor_lr"], critic_lr=t["critic_lr"], alpha_lr=t["alpha_lr"]))
    agent.memory.first_store = False
    env = ops.CartPoleVec(1, seed=1000 + seed)
    out, lens, ep = [], [], 0
    for step in range(1, c["steps"] + 1):
        state = env.obs().copy()
        a = agent.act(state, True)
        nxt, rew, done = env.step(a["action"].reshape(-1))
        agent.process([dict(a, state=state, next_state=np.array(nxt, np.float32), reward=np.asarray(rew, np.float64).reshape(1, 1), done=np.asarray(done).reshape(1, 1).astype(bool))], step)
        ep += 1
        if bool(np.asarray(done).reshape(-1)[0]):
            lens.append(ep)
            ep = 0
        if step % c["chunk"] == 0:
            out.append(float(np.mean(lens)) if lens else float(ep))
            lens = []
    return out


def discrete(args):
    """--discrete: learn() of the discrete SAC next to DQN (tools/bench_mdqn.py's agent at config.dqn.cartpole's shapes, B 32) in the same process,
    alternating; the library's kernel launches of one learn of each (bench_mpo.launches)."""
    import bench_mdqn as M
    import bench_mpo as P

    agents = {"sac_discrete": make_discrete_agent(), "dqn": M.make_agent("dqn", "cartpole")[0]}
    for agent in agents.values():
        T.time_learn(agent, args.warmup)
    learn = {k: [T.time_learn(agent, args.updates) for _ in range(args.rounds)] for k, agent in agents.items()}
    out = {"tool": "tools/bench_sac.py --discrete", "shape": "config.sac.cartpole_discrete (S 4, A 2, H 512, B 64); dqn: config.dqn.cartpole (B 32)",
           "device": torch.cuda.get_device_name(0), "updates": args.updates, "rounds": args.rounds}
    for name, agent in agents.items():
        ms = float(np.median(learn[name])) * 1e3
        per, total = P.launches(agent)
        out[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "launches_per_learn": total, "launches_of_one_learn": per,
                     "learn_in_hipgraph": agent._graph is not None}
    if args.curve:
        with open(os.path.join(ROOT, "tests", "golden", "curves_reference_sac_discrete.json")) as f:
            fx = json.load(f)
        out["cartpole_curves"] = {"config": fx["config"], "hip": [discrete_curve(s, fx["config"]) for s in fx["seeds"]], "reference": fx["sac_discrete"]["reference"]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations sac / td3; the median is reported")
    ap.add_argument("--discrete", action="store_true", help="the discrete SAC at config.sac.cartpole_discrete's shapes next to DQN, with launches per learn")
    ap.add_argument("--curve", action="store_true", help="with --discrete: three seeds of the CartPole curve next to the reference's")
    args = ap.parse_args()
    if args.discrete:
        if not torch.cuda.is_available():
            raise SystemExit("tools/bench_sac.py measures on the GPU: no device found")
        torch.manual_seed(0)
        np.random.seed(0)
        return discrete(args)
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
