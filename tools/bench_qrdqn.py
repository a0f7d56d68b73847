#!/usr/bin/env python3
"""Measurement of the QR-DQN agent (core/agent/qrdqn.py on libjorldy_hip) at two shapes:

  cartpole   config.qrdqn.cartpole: S 4, A 2, hidden 512, B 32, N 200 (400 outputs), Adam 1e-4 eps 1e-2/32
  atari      the config.qrdqn.atari learner: (4, 84, 84) uint8 frames, A 6, hidden 512, B 32, N 200 (1 200 outputs), cnn head

Per shape: learn() in ms and updates/s, and single-mode env steps/s with act() on the GPU every step (epsilon 0: every act() is the
network + jh_quantile_act; one store + one learn() per step as DQN.process does).  In the same process, alternating with it,
Agent("c51") at the same state shape, B and head (51 atoms): the yardstick that exists without this agent.

--cpu adds the reference-equivalent update in torch on the CPU (written here from the formulas of qrdqn.py:60-99), checked against
tests/golden/qrdqn_cartpole.npz to 1e-6 before it is timed.  One JSON line at the end.

    python tools/bench_qrdqn.py [--updates 300] [--steps 300] [--rounds 3] [--shapes cartpole,atari] [--cpu]
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
    "cartpole": dict(state_size=4, action_size=2, head="mlp", optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}),
    "atari": dict(state_size=(4, 84, 84), action_size=6, head="cnn", optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}),
}
FILL = 2048


def make_agent(name, shape):
    from jorldy_amd.core.agent import Agent

    kw = dict(SHAPES[shape], hidden_size=512, gamma=0.99, buffer_size=4096, batch_size=32, start_train_step=0, target_update_period=500, run_step=1_000_000,
              epsilon_init=0.0, epsilon_min=0.0, device="cuda")
    kw.update(dict(num_support=200) if name == "qrdqn" else dict(num_support=51, v_min=-10, v_max=10))
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    S, A = kw["state_size"], kw["action_size"]
    draw = (lambda m: rng.randint(0, 256, size=(m,) + tuple(S), dtype=np.uint8)) if isinstance(S, tuple) else (lambda m: rng.randn(m, S).astype(np.float32))
    cols = {"state": draw(FILL), "action": rng.randint(0, A, size=(FILL, 1)), "reward": rng.choice([0.0, 1.0], size=(FILL, 1)).astype(np.float32),
            "next_state": draw(FILL), "done": rng.rand(FILL, 1) < 0.02}
    agent.memory.store_soa(cols)
    one = [{k: v[i : i + 1] for k, v in cols.items()} for i in range(8)]
    return agent, one


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
    """The reference's update in torch on the CPU: q-network S -> 512 -> 512 -> A N, quantile-Huber loss, Adam."""
    import torch.nn.functional as F

    from oracle import synth

    torch.set_num_threads(threads)
    S, A, H, B, N = (int(z[f"hyper/{k}"]) for k in ("S", "A", "H", "B", "num_support"))
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(S, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(), torch.nn.Linear(H, A * N))
    names = ["head.l.weight", "head.l.bias", "l.weight", "l.bias", "q.weight", "q.bias"]
    net, tgt = mk(), mk()
    seed = int(z["recipe_seed"])
    for m, sd in ((net, seed), (tgt, seed + 1)):
        with torch.no_grad():
            for p, k in zip(m.parameters(), names):
                p.copy_(torch.from_numpy(synth.recipe_tensor(k, tuple(p.shape), sd)))
    opt = torch.optim.Adam(net.parameters(), lr=float(z["hyper/lr"]), eps=float(z["hyper/optim_eps"]))
    tau = torch.from_numpy(z["tau"]).view(1, N)
    inv_tau = 1 - tau
    gamma = float(z["hyper/gamma"])
    s, ns = torch.from_numpy(z["learn/state"]), torch.from_numpy(z["learn/next_state"])
    a, r, d = torch.from_numpy(z["learn/action"]).long().view(B), torch.from_numpy(z["learn/reward"]).float(), torch.from_numpy(z["learn/done"]).float()
    rows = torch.arange(B)

    def update():
        logit = net(s).view(B, A, N)
        pred = logit[rows, a].unsqueeze(1)  # [B, 1, N] (i)
        with torch.no_grad():
            a_star = net(ns).view(B, A, N).mean(-1).argmax(-1)
            target = (r + (1 - d) * gamma * tgt(ns).view(B, A, N)[rows, a_star]).unsqueeze(2)  # [B, N, 1] (j)
        err = target - pred
        hub = F.smooth_l1_loss(*torch.broadcast_tensors(pred, target), reduction="none")
        loss = (torch.where(err < 0.0, inv_tau, tau) * hub).sum(2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.item()

    loss = update()
    ref = float(z["result/loss"])
    assert abs(loss - ref) <= 1e-6 * abs(ref), f"CPU update does not reproduce the fixture: loss {loss!r} vs {ref!r}"
    sd1 = dict(zip(names, net.parameters()))
    for k, p in sd1.items():
        got, want = synth.thin(p.detach().numpy()), z[f"sd1_thin/{k}"]
        assert float(np.abs(got - want).max()) <= 1e-6, f"CPU update does not reproduce the fixture: {k}"
    for _ in range(5):
        update()
    t0 = time.perf_counter()
    n = 50
    for _ in range(n):
        update()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations qrdqn / c51; the median is reported")
    ap.add_argument("--shapes", default="cartpole,atari")
    ap.add_argument("--cpu", action="store_true", help="also time the reference-equivalent torch CPU update (config.qrdqn.cartpole)")
    ap.add_argument("--cpu-threads", type=int, default=8)
    args = ap.parse_args()
    out = {"tool": "tools/bench_qrdqn.py", "updates": args.updates, "steps": args.steps, "rounds": args.rounds, "shapes": {}}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        for shape in args.shapes.split(","):
            agents = {name: make_agent(name, shape) for name in ("qrdqn", "c51")}
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
            res = {}
            for name, (agent, _) in agents.items():
                ms, st = float(np.median(learn[name])) * 1e3, float(np.median(step[name]))
                res[name] = {"learn_ms": round(ms, 4), "updates_per_s": round(1e3 / ms, 1), "env_steps_per_s_single_mode": round(1.0 / st, 1),
                             "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "learn_in_hipgraph": agent._graph is not None,
                             "outputs": int(agent._net.A * agent._net.K)}
            res["qrdqn_over_c51_learn"] = round(res["qrdqn"]["learn_ms"] / res["c51"]["learn_ms"], 3)
            out["shapes"][shape] = res
            del agents
    else:
        out["device"] = None
    if args.cpu:
        z = np.load(os.path.join(ROOT, "tests", "golden", "qrdqn_cartpole.npz"))
        s = cpu_update(z, args.cpu_threads)
        out["cpu_torch_update"] = {"shape": "cartpole", "threads": args.cpu_threads, "update_ms": round(s * 1e3, 3), "updates_per_s": round(1.0 / s, 1),
                                   "checked_against": "tests/golden/qrdqn_cartpole.npz (loss and stepped weights to 1e-6)"}
    line = json.dumps(out)
    assert len(line) < 6000
    print(line)


if __name__ == "__main__":
    main()
