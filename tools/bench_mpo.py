#!/usr/bin/env python3
"""Measurement of the discrete MPO agent (core/agent/mpo.py on libjorldy_hip) at two shapes:

  cartpole   config.mpo.cartpole: S 4, A 2, hidden 512, B 64 trajectories of T 4 (256 rows), n_epoch 16, Adam 2.5e-4
  default    the agent's defaults at the same observation: B 64, T 8 (512 rows), n_epoch 64

Per shape: learn() in ms (the hipGraph replay, statistics read back each time), the library's kernel launches of one learn (counted by its
own per-kernel timers over one eager learn), and single-mode env steps/s: act() on the GPU, interact_callback, one store and n_epoch learns
per env step, as MPO.process does.  In the same process, alternating with it, Agent("dqn") at the same observation and hidden size with
B 64: ONE network, three forwards and one learn per env step, next to MPO's two networks, six forwards and n_epoch learns.  One JSON line.

    python tools/bench_mpo.py [--updates 300] [--steps 60] [--rounds 3] [--shapes cartpole,default] [--continuous [--curve]]

--continuous adds, on the same JSON line, the continuous agent (actor continuous_policy, critic continuous_q_network, num_sample 30) at

  pendulum        config.mpo.pendulum: S 3, A 1, hidden 512, B 64 trajectories of T 4 (256 rows, 7680 sampled rows), Retrace
  hopper_mlagent  config.mpo.hopper_mlagent: S 76, A 3, hidden 512, B 32, 1step_TD (32 rows, 960 sampled rows)

alternating in the same process with the discrete agent at `cartpole`: learn() in ms and the launches of one learn.  --curve adds three seeds of it
on the control env (tests/mpo_cont_truth.py's CURVE_CONFIG) next to the reference's curves of tests/golden/curves_reference_mpo_continuous.json.
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
    "cartpole": dict(batch_size=64, n_step=4, n_epoch=16, eps_eta=0.02, eps_alpha_mu=0.01, eps_alpha_sigma=0.01),
    "default": dict(batch_size=64, n_step=8, n_epoch=64),
}
S, A, FILL = 4, 2, 2048
CONTINUOUS = {
    "pendulum": dict(state_size=3, action_size=1, batch_size=64, n_step=4, n_epoch=64, critic_loss_type="retrace"),
    "hopper_mlagent": dict(state_size=76, action_size=3, batch_size=32, n_step=1, n_epoch=64, critic_loss_type="1step_TD"),
}


def make_continuous(shape):
    from jorldy_amd.core.agent import Agent

    rng = np.random.RandomState(1)
    kw = dict(CONTINUOUS[shape], hidden_size=512, head="mlp", actor="continuous_policy", critic="continuous_q_network", optim_config={"name": "adam", "lr": 2.5e-4},
              gamma=0.99, buffer_size=4096, start_train_step=0, run_step=1_000_000, num_sample=30, device="cuda")
    agent = Agent("mpo", **kw)
    T, s, a = agent.n_step, kw["state_size"], kw["action_size"]
    agent.memory.first_store = False
    agent.memory.store_soa({"state": rng.randn(FILL, T, s).astype(np.float32), "action": np.tanh(rng.randn(FILL, T, a)).astype(np.float32),
                            "reward": rng.choice([0.1, -1.0], size=(FILL, T, 1)).astype(np.float32), "next_state": rng.randn(FILL, T, s).astype(np.float32),
                            "done": rng.rand(FILL, T, 1) < 0.02, "prob": rng.uniform(0.05, 0.7, size=(FILL, T, 1)).astype(np.float32)})
    return agent


def continuous_leg(args):
    """learn() of the continuous agent at the reference's two continuous shapes, the discrete agent at `cartpole` next to it in the same process."""
    res = {}
    discrete, _ = make_agent("mpo", "cartpole")
    time_learn(discrete, args.warmup)
    for shape in CONTINUOUS:
        agent = make_continuous(shape)
        time_learn(agent, args.warmup)
        learn = {"continuous": [], "discrete_cartpole": []}
        for _ in range(args.rounds):
            learn["continuous"].append(time_learn(agent, args.updates))
            learn["discrete_cartpole"].append(time_learn(discrete, args.updates))
        per, total = launches(agent)
        res[shape] = {"learn_ms": round(float(np.median(learn["continuous"])) * 1e3, 4), "rows": agent.batch_size * agent.n_step,
                      "sampled_rows": agent.num_sample * agent.batch_size * agent.n_step, "launches_per_learn": total, "launches_of_one_learn": per,
                      "learn_in_hipgraph": agent._graph is not None, "learn_ms_rounds": [round(v * 1e3, 4) for v in learn["continuous"]],
                      "discrete_cartpole_learn_ms": round(float(np.median(learn["discrete_cartpole"])) * 1e3, 4)}
        del agent
    return res


def make_agent(name, shape):
    from jorldy_amd.core.agent import Agent

    rng = np.random.RandomState(0)
    kw = dict(state_size=S, action_size=A, hidden_size=512, head="mlp", optim_config={"name": "adam", "lr": 2.5e-4}, gamma=0.99, buffer_size=4096, start_train_step=0,
              run_step=1_000_000, device="cuda")
    if name == "mpo":
        kw.update(SHAPES[shape], actor="discrete_policy", critic="discrete_q_network")
        T = kw["n_step"]
        cols = {"state": rng.randn(FILL, T, S).astype(np.float32), "action": rng.randint(0, A, size=(FILL, T, 1)), "reward": rng.choice([0.1, -1.0], size=(FILL, T, 1)).astype(np.float32),
                "next_state": rng.randn(FILL, T, S).astype(np.float32), "done": rng.rand(FILL, T, 1) < 0.02, "prob": rng.uniform(0.3, 0.7, size=(FILL, T, 1)).astype(np.float32)}
    else:
        kw.update(network="discrete_q_network", batch_size=64, target_update_period=500, epsilon_init=0.0, epsilon_min=0.0)
        cols = {"state": rng.randn(FILL, S).astype(np.float32), "action": rng.randint(0, A, size=(FILL, 1)), "reward": rng.choice([0.1, -1.0], size=(FILL, 1)).astype(np.float32),
                "next_state": rng.randn(FILL, S).astype(np.float32), "done": rng.rand(FILL, 1) < 0.02}
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    agent.memory.store_soa(cols)
    one = [{"state": rng.randn(1, S).astype(np.float32), "next_state": rng.randn(1, S).astype(np.float32), "reward": np.asarray([[0.1]]), "done": np.asarray([[False]])} for _ in range(8)]
    return agent, one


def time_learn(agent, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.learn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def time_steps(agent, one, n, step0):
    """act() on the GPU + interact_callback + store + the agent's learns per env step (run_mode.py's single loop without an env behind it)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        tr = dict(one[i % len(one)])
        tr.update(agent.act(tr["state"], True))
        tr = agent.interact_callback(tr)
        if tr:
            agent.process([tr], step0 + i + 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def launches(agent):
    """One learn with the library's per-kernel timers on (it runs eagerly: the timers do not run inside a graph) -> ({kernel: launches}, total)."""
    from jorldy_amd import ops

    ops.lib_profile(True)
    agent.learn()
    torch.cuda.synchronize()
    per = {k: v[0] for k, v in ops.lib_profile_report().items()}
    ops.lib_profile(False)
    return per, sum(per.values())


def continuous_curve():
    """The continuous agent in MPO's single-mode loop on the control env (ops.ControlVec, the oracle's dynamics) at tests/mpo_cont_truth.py's
    CURVE_CONFIG, one curve per seed, next to the unmodified reference's curves of tests/golden/curves_reference_mpo_continuous.json
    (tools/gen_golden_mpo_continuous.py --only curves): first and last tenth of each."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mpo_cont_truth as D

    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    c = D.CURVE_CONFIG
    hip = []
    for seed in c["seeds"]:
        np.random.seed(seed)
        torch.manual_seed(seed)
        agent = Agent("mpo", run_step=c["run_step"], device="cuda", **c["agent"])
        agent.memory.first_store = False
        hip.append([round(v, 4) for v in D.control_curve(agent, ops.ControlVec(1, c["S"], c["A"], seed=1000 + seed), c["steps"], c["bin"])])
    out = {"config": json.loads(json.dumps(c)), "hip": hip, "hip_first_last_tenth": [D.curve_tenths(v) for v in hip]}
    path = os.path.join(D.GOLDEN, "curves_reference_mpo_continuous.json")
    if os.path.exists(path):
        with open(path) as f:
            fx = json.load(f)
        ref = fx["mpo_control"]["reference"]
        out["reference_config_matches"] = fx["config"] == out["config"]
        out["reference_first_last_tenth"] = [D.curve_tenths(v) for v in ref]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations mpo / dqn; the median is reported")
    ap.add_argument("--shapes", default="cartpole,default")
    ap.add_argument("--continuous", action="store_true", help="add the continuous agent at config.mpo.pendulum's and config.mpo.hopper_mlagent's shapes")
    ap.add_argument("--curve", action="store_true", help="with --continuous: three seeds of the continuous agent on the control env next to the reference's curves")
    args = ap.parse_args()
    out = {"tool": "tools/bench_mpo.py", "updates": args.updates, "steps": args.steps, "rounds": args.rounds, "shapes": {}}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        for shape in args.shapes.split(","):
            agents = {name: make_agent(name, shape) for name in ("mpo", "dqn")}
            for agent, one in agents.values():
                time_learn(agent, args.warmup)
                time_steps(agent, one, 10, 0)  # fills MPO's window
            learn = {k: [] for k in agents}
            step = {k: [] for k in agents}
            step0 = 10
            for _ in range(args.rounds):
                for name, (agent, one) in agents.items():
                    learn[name].append(time_learn(agent, args.updates))
                for name, (agent, one) in agents.items():
                    step[name].append(time_steps(agent, one, args.steps, step0))
                step0 += args.steps
            res = {}
            for name, (agent, _) in agents.items():
                ms, st = float(np.median(learn[name])) * 1e3, float(np.median(step[name]))
                per, total = launches(agent)
                res[name] = {"learn_ms": round(ms, 4), "learns_per_env_step": getattr(agent, "n_epoch", 1), "env_steps_per_s_single_mode": round(1.0 / st, 1),
                             "launches_per_learn": total, "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "learn_in_hipgraph": agent._graph is not None}
                if name == "mpo":
                    res[name]["rows"] = agent.batch_size * agent.n_step
                    res[name]["launches_of_one_learn"] = per
            res["mpo_over_dqn_learn"] = round(res["mpo"]["learn_ms"] / res["dqn"]["learn_ms"], 3)
            out["shapes"][shape] = res
            del agents
        if args.continuous:
            out["continuous"] = continuous_leg(args)
            if args.curve:
                out["continuous_curve"] = continuous_curve()
    else:
        out["device"] = None
    line = json.dumps(out)
    print(line)


if __name__ == "__main__":
    main()
