#!/usr/bin/env python3
"""Measurement of the IQN agent (core/agent/iqn.py on libjorldy_hip) at config.iqn.cartpole shapes: S 4, A 2, width 512, B 32,
N 64 samples, E 64 cosine features, Adam 1e-4 eps 1e-2/32 -- 2 048 network rows per forward, 6 144 per learn().

learn() in ms and updates/s, and single-mode env steps/s with act() on the GPU every step (epsilon 0: every act() is the network +
jh_iqn_act; one store + one learn() per step as DQN.process does).  In the same process, alternating with it, Agent("qrdqn") at
config.qrdqn.cartpole shapes (N 200 on the q-network): the distributional yardstick that exists without this agent.

--cpu adds the same update in torch on the CPU (float32, written here from the formulas of network/iqn.py:26-47 and agent/iqn.py:78-129),
checked against tests/golden/iqn_cartpole.npz before it is timed.  Reads nothing from the reference.  One JSON line at the end.

    python tools/bench_iqn.py [--updates 300] [--steps 300] [--rounds 3] [--cpu]
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

FILL = 2048
KEYS = ("head.l", "state_embed", "sample_embed", "l1", "l2", "q")


def make_agent(name):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=4, action_size=2, optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}, gamma=0.99, buffer_size=4096, batch_size=32,
              start_train_step=0, target_update_period=500, run_step=1_000_000, epsilon_init=0.0, epsilon_min=0.0, device="cuda")
    kw.update(dict(num_sample=64, embedding_dim=64) if name == "iqn" else dict(num_support=200, hidden_size=512))
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    cols = {"state": rng.randn(FILL, 4).astype(np.float32), "action": rng.randint(0, 2, size=(FILL, 1)), "reward": rng.choice([0.0, 1.0], size=(FILL, 1)).astype(np.float32),
            "next_state": rng.randn(FILL, 4).astype(np.float32), "done": rng.rand(FILL, 1) < 0.02}
    agent.memory.store_soa(cols)
    return agent, [{k: v[i : i + 1] for k, v in cols.items()} for i in range(8)]


def time_learn(agent, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        agent.learn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def time_steps(agent, one, n, step0):
    """act() on the GPU + store + learn() per env step (run_mode.py:68-91 without an env behind it)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        tr = dict(one[i % len(one)])
        tr.update(agent.act(tr["state"], True))
        agent.process([tr], step0 + i + 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def cpu_update(z, threads):
    """The same update in torch on the CPU, float32: the three forwards with their own tau draws, quantile-Huber loss, Adam."""
    import torch.nn.functional as F

    from oracle import synth

    torch.set_num_threads(threads)
    B, N, A, E = (int(z[f"hyper/{k}"]) for k in ("B", "N", "A", "E"))
    seed, gamma = int(z["recipe_seed"]), float(z["hyper/gamma"])
    shapes = {k[6:]: tuple(int(v) for v in z[k]) for k in z.files if k.startswith("shape/")}
    net, tgt = ({k: torch.from_numpy(v).requires_grad_(s == seed) for k, v in synth.recipe_state_dict(shapes, s).items()} for s in (seed, seed + 1))
    opt = torch.optim.Adam(list(net.values()), lr=float(z["hyper/lr"]), eps=float(z["hyper/optim_eps"]))
    i_pi = (torch.arange(0, E) * np.pi).view(1, 1, E)
    s, ns = torch.from_numpy(z["learn/state"]), torch.from_numpy(z["learn/next_state"])
    a, r, d = torch.from_numpy(z["learn/action"]).long().view(B), torch.from_numpy(z["learn/reward"]).float(), torch.from_numpy(z["learn/done"]).float()
    rows = torch.arange(B)

    def forward(w, x, tau):
        lin = lambda k, v: F.linear(v, w[k + ".weight"], w[k + ".bias"])
        psi = F.relu(lin("state_embed", F.relu(lin("head.l", x))))
        phi = F.relu(lin("sample_embed", torch.cos(tau.unsqueeze(-1) * i_pi)))
        return lin("q", F.relu(lin("l2", F.relu(lin("l1", psi.unsqueeze(1) * phi)))))

    def update(taus):
        logit = forward(net, s, taus[0])  # [B, N, A]
        pred = logit[rows, :, a].unsqueeze(1)  # [B, 1, N] (i)
        with torch.no_grad():
            a_star = forward(net, ns, taus[1]).mean(1).argmax(-1)
            target = (r + (1 - d) * gamma * forward(tgt, ns, taus[2])[rows, :, a_star]).unsqueeze(2)  # [B, N, 1] (j)
        err = target - pred
        hub = F.smooth_l1_loss(*torch.broadcast_tensors(pred, target), reduction="none")
        tau = taus[0].unsqueeze(1)
        loss = (torch.where(err < 0.0, 1 - tau, tau) * hub).sum(2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.item()

    loss = update(torch.from_numpy(z["learn/tau"]))
    ref = float(z["result/loss"])
    assert abs(loss - ref) <= 1e-5 * abs(ref), f"CPU update does not reproduce the fixture: loss {loss!r} vs {ref!r}"
    for _ in range(3):
        update(torch.rand(3, B, N))
    t0 = time.perf_counter()
    n = 20
    for _ in range(n):
        update(torch.rand(3, B, N))
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations iqn / qrdqn; the median is reported")
    ap.add_argument("--cpu", action="store_true", help="also time the same update in torch on the CPU (config.iqn.cartpole)")
    ap.add_argument("--cpu-threads", type=int, default=8)
    args = ap.parse_args()
    out = {"tool": "tools/bench_iqn.py", "shape": "config.iqn.cartpole", "updates": args.updates, "steps": args.steps, "rounds": args.rounds}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        agents = {name: make_agent(name) for name in ("iqn", "qrdqn")}
        for agent, _ in agents.values():
            time_learn(agent, args.warmup)
        learn = {k: [] for k in agents}
        step = {k: [] for k in agents}
        step0 = 0
        for _ in range(args.rounds):
            for name, (agent, one) in agents.items():
                learn[name].append(time_learn(agent, args.updates))
            for name, (agent, one) in agents.items():
                step[name].append(time_steps(agent, one, args.steps, step0))
            step0 += args.steps
        for name, (agent, _) in agents.items():
            ms, st = float(np.median(learn[name])) * 1e3, float(np.median(step[name]))
            out[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "env_steps_per_s_single_mode": round(1.0 / st, 1),
                         "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "learn_in_hipgraph": agent._graph is not None,
                         "rows_per_forward": int(32 * agent._net.K) if name == "iqn" else 32}
        out["iqn_over_qrdqn_learn"] = round(out["iqn"]["learn_ms"] / out["qrdqn"]["learn_ms"], 3)
    else:
        out["device"] = None
    if args.cpu:
        z = np.load(os.path.join(ROOT, "tests", "golden", "iqn_cartpole.npz"))
        s = cpu_update(z, args.cpu_threads)
        out["cpu_torch_update"] = {"threads": args.cpu_threads, "update_ms": round(s * 1e3, 3), "updates_per_s": round(1.0 / s, 1),
                                   "checked_against": "tests/golden/iqn_cartpole.npz (loss to 1e-5)"}
    line = json.dumps(out)
    assert len(line) < 6000
    print(line)


if __name__ == "__main__":
    main()
