#!/usr/bin/env python3
"""Measurement of the ICM-PPO agent (core/agent/icm_ppo.py on libjorldy_hip) at config.icm_ppo.cartpole's shapes: S 4, A 2, H 512, 8 workers x
128 steps = 1024 rows, B 32, 3 epochs = 96 PPO updates + 96 ICM updates per learn(), Adam 2.5e-4.

learn() in ms (whole process(): store of the rollout, the captured graph's replay, the statistics' arrival) for ICM-PPO and, in the same
process at the same shapes, for PPO; the two alternate and the median of the rounds is reported, so `icm_half_ms` = ICM-PPO - PPO is what
the curiosity module costs (its no-grad pass over the rollout and its 96 updates).  `launches_per_icm_update` is counted, not assumed: one
eager jh_icmnet_update under the library's per-kernel profile, which also gives the share of each kernel of that update.
Reads nothing from the reference.  One JSON line at the end.

    python tools/bench_icm_ppo.py [--learns 30] [--rounds 5]
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

S, A, H, W, T, B, E = 4, 2, 512, 8, 128, 32, 3
PPO_KW = dict(state_size=S, action_size=A, hidden_size=H, network="discrete_policy_value", head="mlp", optim_config={"name": "adam", "lr": 2.5e-4}, gamma=0.99, batch_size=B,
              n_step=T, n_epoch=E, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, clip_grad_norm=1.0, use_standardization=False, lr_decay=True,
              run_step=10_000_000, num_workers=W, device="cuda")
ICM_KW = dict(icm_network="icm_mlp", beta=0.2, lamb=1.0, eta=0.1, extrinsic_coeff=1.0, intrinsic_coeff=1.0)


def rollout(seed):
    rng = np.random.RandomState(seed)
    M = W * T
    return {"state": rng.randn(M, S).astype(np.float32), "next_state": rng.randn(M, S).astype(np.float32), "reward": rng.randn(M, 1).astype(np.float32),
            "done": (rng.rand(M, 1) < 0.02).astype(np.float32), "action": rng.randint(0, A, size=(M, 1)).astype(np.float32)}


def make(name):
    from jorldy_amd.core.agent import Agent

    agent = Agent(name, **PPO_KW, **(ICM_KW if name == "icm_ppo" else {}))
    agent.memory.first_store = False
    return agent


def time_learns(agent, cols, n, step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step += T
        agent.process(cols[i % len(cols)], step)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, step


def count_update_launches():
    """One eager jh_icmnet_update at the bench's shapes under the per-kernel profile.  -> (launches, {kernel: (launches, us)})"""
    from jorldy_amd import ops

    net = ops.ICMNet(S, H, A, False, W, W * T, "cuda", eta=0.1, gamma=0.99)
    with torch.no_grad():
        for k, v in net._pairs(net.params):
            v.copy_(torch.ones_like(v) if k.startswith("bn") and k.endswith("weight") else 0.05 * torch.randn_like(v))
    net.set_hyper(2.5e-4)
    c = {k: torch.from_numpy(v).cuda() for k, v in rollout(9).items()}
    idx = torch.randperm(W * T, device="cuda")[:B]
    for _ in range(3):
        net.update(c["state"], c["next_state"], c["action"], idx, 0.2, 1.0)
    torch.cuda.synchronize()
    ops.lib_profile(True)
    reps = 20
    for _ in range(reps):
        net.update(c["state"], c["next_state"], c["action"], idx, 0.2, 1.0)
    rep = ops.lib_profile_report()
    ops.lib_profile(False)
    rep = {k: v for k, v in rep.items() if not k.startswith("__")}
    return sum(v[0] for v in rep.values()) // reps, {k: (v[0] // reps, round(1e3 * v[1] / reps, 2)) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learns", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    np.random.seed(0)
    cols = [rollout(s) for s in range(4)]
    agents = {"icm_ppo": make("icm_ppo"), "ppo": make("ppo")}
    steps = {k: 0 for k in agents}
    for k, a in agents.items():  # warm-up: eager learn, capture, first replays
        _, steps[k] = time_learns(a, cols, 6, steps[k])
    ms = {k: [] for k in agents}
    for _ in range(args.rounds):
        for k, a in agents.items():
            t, steps[k] = time_learns(a, cols, args.learns, steps[k])
            ms[k].append(1e3 * t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    launches, kernels = count_update_launches()
    n_upd = E * (W * T // B)
    print(json.dumps({"bench": "icm_ppo", "device": torch.cuda.get_device_name(0), "shapes": {"S": S, "A": A, "H": H, "rows": W * T, "B": B, "epochs": E, "updates": n_upd},
                      "icm_ppo_learn_ms": round(med["icm_ppo"], 3), "ppo_learn_ms": round(med["ppo"], 3), "icm_half_ms": round(med["icm_ppo"] - med["ppo"], 3),
                      "icm_over_ppo": round(med["icm_ppo"] / med["ppo"], 3), "icm_us_per_update": round(1e3 * (med["icm_ppo"] - med["ppo"]) / n_upd, 2),
                      "captured": {k: bool(a._graphs) for k, a in agents.items()}, "launches_per_icm_update": launches, "icm_update_kernels_launches_us": kernels, "rounds_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
