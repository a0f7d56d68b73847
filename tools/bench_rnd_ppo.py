#!/usr/bin/env python3
"""Measurement of the RND-PPO agent (core/agent/rnd_ppo.py on libjorldy_hip) at config.rnd_ppo.cartpole's shapes: S 4, A 2, H 512, 8 workers x
128 steps = 1024 rows, B 64, 3 epochs = 48 policy updates + 48 module updates per learn(), Adam 1e-4.

learn() in ms (whole process(): store of the rollout, the captured graph's replay, the statistics' read-back) for RND-PPO and, in the same
process at the same shapes, for PPO and ICM-PPO (each with its own network: one value head); the three alternate and the median of the
rounds is reported.  `launches_per_rnd_update` is counted, not assumed: one eager jh_rndnet_update under the library's per-kernel profile,
which also gives the share of each kernel of that update; ICM's is counted beside it.  --curve adds CartPole curves (ops.CartPoleVec,
config.rnd_ppo.cartpole, 40 iterations) for the given seeds.  Reads nothing from the reference.  One JSON line at the end.

    python tools/bench_rnd_ppo.py [--learns 30] [--rounds 5] [--curve 1,2,3]
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

S, A, H, W, T, B, E = 4, 2, 512, 8, 128, 64, 3
BASE = dict(state_size=S, action_size=A, hidden_size=H, head="mlp", optim_config={"name": "adam", "lr": 1e-4}, gamma=0.99, batch_size=B, n_step=T, n_epoch=E, _lambda=0.95,
            epsilon_clip=0.1, vf_coef=0.5, ent_coef=0.01, clip_grad_norm=1.0, use_standardization=False, lr_decay=True, run_step=10_000_000, num_workers=W, device="cuda")
EXTRA = {"ppo": dict(network="discrete_policy_value"),
         "icm_ppo": dict(network="discrete_policy_value", icm_network="icm_mlp", beta=0.2, lamb=1.0, eta=0.1, extrinsic_coeff=1.0, intrinsic_coeff=1.0),
         "rnd_ppo": dict(network="discrete_policy_separate_value", rnd_network="rnd_mlp", gamma_i=0.99, extrinsic_coeff=2.0, intrinsic_coeff=1.0, obs_normalize=True,
                         ri_normalize=True, batch_norm=True, non_episodic=False)}


def rollout(seed):
    rng = np.random.RandomState(seed)
    M = W * T
    return {"state": rng.randn(M, S).astype(np.float32), "next_state": rng.randn(M, S).astype(np.float32), "reward": rng.randn(M, 1).astype(np.float32),
            "done": (rng.rand(M, 1) < 0.02).astype(np.float32), "action": rng.randint(0, A, size=(M, 1)).astype(np.float32)}


def make(name, **over):
    from jorldy_amd.core.agent import Agent

    agent = Agent(name, **{**BASE, **EXTRA[name], **over})
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


def count_update_launches(which):
    """One eager module update at the bench's shapes under the per-kernel profile.  -> (launches, {kernel: (launches, us)})"""
    from jorldy_amd import ops

    net = ops.RNDNet(S, H, W, W * T, "cuda") if which == "rnd" else ops.ICMNet(S, H, A, False, W, W * T, "cuda", eta=0.1, gamma=0.99)
    with torch.no_grad():
        for k, v in net._pairs(net.params):
            v.copy_(torch.ones_like(v) if k.startswith("bn") and k.endswith("weight") else 0.05 * torch.randn_like(v))
    net.set_hyper(1e-4)
    c = {k: torch.from_numpy(v).cuda() for k, v in rollout(9).items()}
    idx = torch.randperm(W * T, device="cuda")[:B]
    update = (lambda: net.update(c["next_state"], idx, 1.0)) if which == "rnd" else (lambda: net.update(c["state"], c["next_state"], c["action"], idx, 0.2, 1.0))
    for _ in range(3):
        update()
    torch.cuda.synchronize()
    ops.lib_profile(True)
    reps = 20
    for _ in range(reps):
        update()
    rep = ops.lib_profile_report()
    ops.lib_profile(False)
    rep = {k: v for k, v in rep.items() if not k.startswith("__")}
    return sum(v[0] for v in rep.values()) // reps, {k: (v[0] // reps, round(1e3 * v[1] / reps, 2)) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1])}


def curve(seed, iterations=40):
    """Mean episode length per iteration on ops.CartPoleVec (the loop of tests/test_rnd_gpu.py's curve test)."""
    from jorldy_amd import ops

    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = make("rnd_ppo", run_step=100000, seed=seed)
    env = ops.CartPoleVec(W, seed=1000 + seed)
    out, step = [], 0
    s_, n_ = np.empty((T, W, 4), np.float32), np.empty((T, W, 4), np.float32)
    a_, r_, d_ = np.empty((T, W, 1), np.float32), np.empty((T, W, 1), np.float32), np.empty((T, W, 1), np.float32)
    for _ in range(iterations):
        for t in range(T):
            s_[t] = env.obs()
            a = agent.act(s_[t], True)["action"]
            nxt, rew, done = env.step(a)
            n_[t], a_[t], r_[t, :, 0], d_[t, :, 0] = nxt, np.asarray(a, dtype=np.float32).reshape(W, 1), rew, done
        wm = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2).reshape(W * T, -1))
        out.append(round(W * T / max(1, int(d_.sum())), 1))
        step += T
        agent.process({"state": wm(s_), "action": wm(a_), "reward": wm(r_), "next_state": wm(n_), "done": wm(d_)}, step)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--learns", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--curve", default="", help="comma-separated seeds: also run CartPole curves")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    torch.manual_seed(0)
    np.random.seed(0)
    cols = [rollout(s) for s in range(4)]
    agents = {k: make(k) for k in ("rnd_ppo", "ppo", "icm_ppo")}
    steps = {k: 0 for k in agents}
    for k, a in agents.items():  # warm-up: eager learn, capture, first replays
        _, steps[k] = time_learns(a, cols, 6, steps[k])
    ms = {k: [] for k in agents}
    for _ in range(args.rounds):
        for k, a in agents.items():
            t, steps[k] = time_learns(a, cols, args.learns, steps[k])
            ms[k].append(1e3 * t)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    captured = {k: bool(a._graphs) for k, a in agents.items()}
    del agents
    launches, kernels = count_update_launches("rnd")
    icm_launches, _ = count_update_launches("icm")
    n_upd = E * (W * T // B)
    out = {"bench": "rnd_ppo", "device": torch.cuda.get_device_name(0), "shapes": {"S": S, "A": A, "H": H, "rows": W * T, "B": B, "epochs": E, "updates": n_upd},
           "rnd_ppo_learn_ms": round(med["rnd_ppo"], 3), "ppo_learn_ms": round(med["ppo"], 3), "icm_ppo_learn_ms": round(med["icm_ppo"], 3),
           "rnd_over_ppo": round(med["rnd_ppo"] / med["ppo"], 3), "rnd_over_icm": round(med["rnd_ppo"] / med["icm_ppo"], 3), "captured": captured,
           "launches_per_rnd_update": launches, "launches_per_icm_update": icm_launches, "rnd_update_kernels_launches_us": kernels,
           "rounds_ms": {k: [round(x, 3) for x in v] for k, v in ms.items()}}
    if args.curve:
        out["curves"] = {s: curve(int(s)) for s in args.curve.split(",")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
