#!/usr/bin/env python3
"""Device-resident rollouts (manager.DeviceCollector, csrc/jh_devroll.hip) against the host-loop collector (NativeCollector) in one process:
env transitions per second of the rollout alone and of rollout + learn().

  cartpole legs   config.ppo.cartpole's shapes (S 4, A 2, H 512, minibatch 256, 3 epochs): W = 8 x T = 128 on both collectors, then the device
                  collector at W = 256 / 1024 / 4096 with T = 128 / 32 / 8 (32 768 rows per learn() each)
  control legs    config.ppo.mujoco's Hopper shapes on the synthetic control env (S 11, A 3, H 512, minibatch 2048, 10 epochs): W = 32 x T = 2048 on
                  both collectors, then the device collector at W = 1024 x T = 64 (65 536 rows each)

Every figure is a host clock around `iters` iterations that end in a device synchronise, after `warmup` untimed iterations (the fourth
captures learn()'s graph).  Prints one JSON line.

    python tools/bench_device_rollout.py [--iters 10] [--warmup 4]

--agent td3 | sac: the device-resident actors of the continuous off-policy agents (csrc/jh_devroll_ac.hip) at config.td3.mujoco / config.sac.mujoco
shapes (S 11, A 3, H 512; batch 128 / 256) on the synthetic control env at W = 32, 256 and 1024: rollout of T = 4 alone, and rollout of T = 4 + one
process(), on DeviceCollector and -- in the same process -- on the agent's own act() loop over ops.ControlVec of the same W (VecCollector).

--agent sac_discrete | dqn: the device-resident actors of the discrete SAC and of DQN (csrc/jh_devroll_disc.hip) at config.sac.cartpole_discrete /
config.dqn.cartpole shapes (S 4, A 2, H 512; batch 64 / 32) on CartPole, the same legs: DeviceCollector on ops.DeviceCartPole next to the agent's own
act() loop over ops.CartPoleVec.  DQN's epsilon starts at 0.1, not the config's 1.0: at 1.0 the host act() never runs its network.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def leg(kind, device_side, W, T, iters, warmup):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import DeviceCollector, NativeCollector

    cont = kind == "control"
    S, A, B, E, lr = (11, 3, 2048, 10, 3e-4) if cont else (4, 2, 256, 3, 2.5e-4)
    torch.manual_seed(0)
    np.random.seed(0)
    agent = Agent("ppo", state_size=S, action_size=A, hidden_size=512, network="continuous_policy_value" if cont else "discrete_policy_value",
                  optim_config={"name": "adam", "lr": lr}, gamma=0.99, batch_size=B, n_step=T, n_epoch=E, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01,
                  clip_grad_norm=1.0, use_standardization=True, lr_decay=True, run_step=1_000_000_000, num_workers=W, device="cuda")
    agent.memory.first_store = False
    if device_side:
        env = ops.DeviceControl(W, S, A, 1, "cuda") if cont else ops.DeviceCartPole(W, 1, "cuda")
        col = DeviceCollector(env, agent, W)
    else:
        col = NativeCollector(ops.ControlVec(W, S, A, seed=1) if cont else ops.CartPoleVec(W, seed=1), agent, W)
    step = 0

    def rollout_only():
        col.run(T)
        agent.memory._store.clear()  # what learn() does with the rows; the capture stays unused
        agent._captured = 0

    def both():
        nonlocal step
        step += T
        col.run(T)
        return agent.process(None, step)

    out = {"collector": type(col).__name__, "env": kind, "W": W, "T": T, "rows_per_iteration": W * T}
    for name, fn in (("rollout", rollout_only), ("rollout_and_learn", both)):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        out[name + "_ms"] = round(dt * 1e3, 4)
        out[name + "_transitions_per_s"] = round(W * T / dt, 1)
    col.terminate()
    return out


def leg_ac(name, device_side, W, T, iters, warmup):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import DeviceCollector, VecCollector

    S, A = 11, 3
    torch.manual_seed(0)
    np.random.seed(0)
    common = dict(hidden_size=512, buffer_size=50000, start_train_step=0, run_step=1_000_000_000, device="cuda")
    if name in ("sac_discrete", "dqn"):  # config.sac.cartpole_discrete / config.dqn.cartpole on the CartPole envs
        S, A = 4, 2
        own = (dict(actor="discrete_policy", critic="discrete_q_network", use_dynamic_alpha=True, batch_size=64, target_update_period=500,
                    optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 1.5e-4, "critic_lr": 3e-4, "alpha_lr": 1e-5}) if name == "sac_discrete" else
               dict(network="discrete_q_network", epsilon_init=0.1, epsilon_min=0.01, explore_ratio=0.2, batch_size=32, target_update_period=500, optim_config={"name": "adam", "lr": 1e-4}))
        agent = Agent("sac" if name == "sac_discrete" else "dqn", state_size=S, action_size=A, **common, **own)
        col = DeviceCollector(ops.DeviceCartPole(W, 1, "cuda"), agent) if device_side else VecCollector(ops.CartPoleVec(W, seed=1), agent)
    else:
        agent = Agent(name, state_size=S, action_size=A, batch_size=128 if name == "td3" else 256, **common)
        col = DeviceCollector(ops.DeviceControl(W, S, A, 1, "cuda"), agent) if device_side else VecCollector(ops.ControlVec(W, S, A, seed=1), agent)
    step = 0

    def both():
        nonlocal step
        step += T
        return agent.process(col.run(T)[0], step)

    out = {"collector": type(col).__name__, "agent": name, "W": W, "T": T, "rows_per_iteration": W * T}
    for key, fn in (("rollout", lambda: col.run(T)), ("rollout_and_learn", both)):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
        out[key + "_ms"] = round(dt * 1e3, 4)
        out[key + "_transitions_per_s"] = round(W * T / dt, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--agent", choices=("ppo", "td3", "sac", "sac_discrete", "dqn"), default="ppo")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured without one"
    if args.agent != "ppo":
        print(json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
                          "legs": [leg_ac(args.agent, d, W, 4, args.iters, args.warmup) for W in (32, 256, 1024) for d in (False, True)]}))
        return
    plan = [("cartpole", False, 8, 128), ("cartpole", True, 8, 128), ("cartpole", True, 256, 128), ("cartpole", True, 1024, 32), ("cartpole", True, 4096, 8),
            ("control", False, 32, 2048), ("control", True, 32, 2048), ("control", True, 1024, 64)]
    print(json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup,
                      "legs": [leg(k, d, W, T, args.iters, args.warmup) for k, d, W, T in plan]}))


if __name__ == "__main__":
    main()
