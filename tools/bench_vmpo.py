#!/usr/bin/env python3
"""Measurement of the V-MPO agent (core/agent/vmpo.py on libjorldy_hip) at the reference's two configurations --
config.vmpo.cartpole (S 4, A 2 discrete, H 512, 8 workers x 128 steps = 1024 rows, minibatches of 64: 16 updates per learn) and
config.vmpo.mujoco (S 11, A 3 continuous, H 512, 4 x 128 = 512 rows, minibatches of 64: 8 updates) -- next to PPO with n_epoch = 1 at the same
shapes in the same process, on both of PPO's update paths: the fused four-launch update (its default at these shapes) and the separate
forward / loss / backward / clip + Adam calls (JH_FUSED_UPDATE=0), which is the path V-MPO's update has the shape of.

learn() in ms (process() of an uploaded synthetic rollout: store, pre-pass, every minibatch update, statistics; one hipGraph once warm), the
agents alternating, the median of the rounds; launches per minibatch update, counted by the library's own per-kernel timers over one learn.
Reads nothing from the reference.  One JSON line at the end.

    python tools/bench_vmpo.py [--iters 30] [--rounds 3]
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
    "cartpole": dict(S=4, A=2, cont=False, W=8, T=128, B=64, lr=2.5e-4, vmpo=dict(eps_eta=0.02, eps_alpha_mu=0.1, eps_alpha_sigma=0.1, eta=2.0, alpha_mu=0.1, alpha_sigma=5.0)),
    "mujoco": dict(S=11, A=3, cont=True, W=4, T=128, B=64, lr=5e-4, vmpo=dict(eps_eta=0.01, eps_alpha_mu=0.01, eps_alpha_sigma=5e-5, eta=1.0, alpha_mu=1.0, alpha_sigma=1.0)),
}


def make(kind, c):
    from jorldy_amd.core.agent import Agent

    common = dict(state_size=c["S"], action_size=c["A"], hidden_size=512, network="continuous_policy_value" if c["cont"] else "discrete_policy_value",
                  optim_config={"name": "adam", "lr": c["lr"]}, gamma=0.99, batch_size=c["B"], n_step=c["T"], n_epoch=1, _lambda=0.95, clip_grad_norm=1.0,
                  lr_decay=True, run_step=1_000_000_000, num_workers=c["W"], device="cuda")
    if kind == "vmpo":
        agent = Agent("vmpo", **common, **c["vmpo"])
    else:
        os.environ["JH_FUSED_UPDATE"] = "0" if kind == "ppo_separate" else "1"  # read at construction
        agent = Agent("ppo", epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, **common)
        os.environ.pop("JH_FUSED_UPDATE", None)
    agent.memory.first_store = False
    return agent


def rollout(c):
    rng = np.random.RandomState(0)
    M, S, A = c["W"] * c["T"], c["S"], c["A"]
    action = np.tanh(rng.randn(M, A)).astype(np.float32) if c["cont"] else rng.randint(0, A, size=(M, 1))
    return {"state": rng.randn(M, S).astype(np.float32), "action": action, "reward": rng.randn(M, 1).astype(np.float32),
            "next_state": rng.randn(M, S).astype(np.float32), "done": (rng.rand(M, 1) < 0.02)}


class Leg:
    def __init__(self, kind, c):
        self.agent, self.cols, self.T, self.step = make(kind, c), rollout(c), c["T"], 0

    def run(self, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.step += self.T
            self.agent.process(self.cols, self.step)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    def launches(self, n_upd):
        """One learn with the library's per-kernel timers on (it runs eagerly: the timers do not run inside a graph) -> ({kernel: launches},
        {kernel: average us}, launches per minibatch update: the kernels launched at least once per update, i.e. everything but the pre-pass)."""
        from jorldy_amd import ops

        ops.lib_profile(True)
        self.step += self.T
        self.agent.process(self.cols, self.step)
        torch.cuda.synchronize()
        prof = ops.lib_profile_report()
        ops.lib_profile(False)
        per = {k: v[0] for k, v in prof.items()}
        us = {k: round(v[1] / v[0] * 1e3, 2) for k, v in prof.items()}
        # a kernel that runs once per minibatch update is launched a multiple of n_upd times; the pre-pass kernels are not
        per_update = sum(n // n_upd for k, n in per.items() if n >= n_upd)
        return per, us, per_update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6, help="untimed learns per agent: eager warm-ups and the captures of the split and the whole-learn graph")
    ap.add_argument("--rounds", type=int, default=3, help="alternations over the agents; the median is reported")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_vmpo.py measures on the GPU: no device found")
    out = {"tool": "tools/bench_vmpo.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds}
    torch.manual_seed(0)
    np.random.seed(0)
    for shape, c in SHAPES.items():
        n_upd = (c["W"] * c["T"]) // c["B"]
        legs = {k: Leg(k, c) for k in ("vmpo", "ppo_fused", "ppo_separate")}
        for leg in legs.values():
            leg.run(args.warmup)
        times = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, leg in legs.items():
                times[k].append(leg.run(args.iters))
        res = {"shape": f"config.vmpo.{shape}: S {c['S']}, A {c['A']} {'continuous' if c['cont'] else 'discrete'}, H 512, {c['W']} x {c['T']} rows, minibatches of {c['B']}",
               "updates_per_learn": n_upd}
        for k, leg in legs.items():
            ms = float(np.median(times[k])) * 1e3
            per, us, per_update = leg.launches(n_upd)
            res[k] = {"learn_ms": round(ms, 4), "ms_per_update": round(ms / n_upd, 4), "learn_ms_rounds": [round(v * 1e3, 4) for v in times[k]],
                      "launches_per_minibatch_update": per_update, "launches_of_one_learn": per, "kernel_avg_us": us, "hipgraphs": len(getattr(leg.agent, "_graphs", {}))}
        out[shape] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
