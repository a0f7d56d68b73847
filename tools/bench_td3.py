#!/usr/bin/env python3
"""Measurement of the TD3 and DDPG agents (core/agent/td3.py, core/agent/ddpg.py on libjorldy_hip) at config.td3.mujoco's shapes: S 11, A 3,
H 512, B 128, Adam 3e-4 (TD3) / 5e-4 and 1e-3 (DDPG).

learn() in ms and updates/s (TD3: the mean over its alternation of critics-only learns and learns with an actor step and a soft update),
and single-mode env steps/s with act() on the GPU every step (one store + one learn() per step as process() does; DDPG's soft update
included).  TD3 and DDPG alternate in the same process; the median of the rounds is reported.

--cpu adds the same updates in torch on the CPU (float32, written here from the formulas of network/policy.py:8-20,
network/q_network.py:23-39, agent/td3.py:146-209 and agent/ddpg.py:117-163), checked against tests/golden/td3.npz before they are timed.
Reads nothing from the reference.  One JSON line at the end.

    python tools/bench_td3.py [--updates 300] [--steps 300] [--rounds 3] [--cpu]
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

S, A, H, B, FILL = 11, 3, 512, 128, 4096
OPT = {"td3": {"actor": "adam", "critic": "adam", "actor_lr": 3e-4, "critic_lr": 3e-4}, "ddpg": {"actor": "adam", "critic": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3}}


def make_agent(name):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=S, action_size=A, hidden_size=H, optim_config=OPT[name], gamma=0.99, buffer_size=8192, batch_size=B, start_train_step=0, tau=5e-3,
              run_step=1_000_000, device="cuda")
    agent = Agent(name, **kw)
    agent.memory.first_store = False
    rng = np.random.RandomState(0)
    cols = {"state": rng.randn(FILL, S).astype(np.float32), "action": np.tanh(rng.randn(FILL, A)).astype(np.float32),
            "reward": rng.randn(FILL, 1).astype(np.float32), "next_state": rng.randn(FILL, S).astype(np.float32), "done": rng.rand(FILL, 1) < 0.02}
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


# ---------------------------------------------------------------------------------------------- the same updates in torch on the CPU
class _Net(torch.nn.Module):
    def __init__(self, s, a, h, critic):
        super().__init__()
        self.head = torch.nn.Module()
        self.head.l = torch.nn.Linear(s, h)
        if critic:
            self.e, self.l, self.q = torch.nn.Linear(a, h), torch.nn.Linear(2 * h, h), torch.nn.Linear(h, 1)
        else:
            self.l, self.pi = torch.nn.Linear(h, h), torch.nn.Linear(h, a)

    def forward(self, x, a=None):
        x = torch.relu(self.head.l(x))
        if a is None:
            return torch.tanh(self.pi(torch.relu(self.l(x))))
        return self.q(torch.relu(self.l(torch.cat([x, torch.relu(self.e(a))], -1))))


class CpuAgent:
    def __init__(self, s, a, h, n_critics, lr_a, lr_c, tau=5e-3, gamma=0.99, std=0.2, clip=0.5, delay=2):
        self.nc, self.tau, self.gamma, self.std, self.clip, self.delay, self.num_learn = n_critics, tau, gamma, std, clip, delay, 0
        self.actor, self.t_actor = _Net(s, a, h, False), _Net(s, a, h, False)
        self.critics, self.t_critics = [_Net(s, a, h, True) for _ in range(n_critics)], [_Net(s, a, h, True) for _ in range(n_critics)]
        self.t_actor.load_state_dict(self.actor.state_dict())
        for c, t in zip(self.critics, self.t_critics):
            t.load_state_dict(c.state_dict())
        self.a_opt = torch.optim.Adam(self.actor.parameters(), lr=lr_a)
        self.c_opts = [torch.optim.Adam(c.parameters(), lr=lr_c) for c in self.critics]

    def soft(self):
        with torch.no_grad():
            for src, dst in [(self.actor, self.t_actor)] + list(zip(self.critics, self.t_critics)):
                for p, t in zip(src.parameters(), dst.parameters()):
                    t.copy_(self.tau * p + (1 - self.tau) * t)

    def learn(self, s, a, r, s2, d, eps=None):
        with torch.no_grad():
            a2 = self.t_actor(s2)
            if self.nc == 2:
                eps = torch.randn_like(a) if eps is None else eps
                a2 = (a2 + (eps * self.std).clamp(-self.clip, self.clip)).clamp(-1.0, 1.0)
            y = r + (1 - d) * self.gamma * torch.stack([t(s2, a2) for t in self.t_critics]).min(0).values
        losses = []
        for c, opt in zip(self.critics, self.c_opts):
            loss = torch.nn.functional.mse_loss(y, c(s, a))
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        if self.nc == 1 or self.num_learn % self.delay == 0:
            al = -self.critics[0](s, self.actor(s)).mean()
            self.a_opt.zero_grad(set_to_none=True)
            al.backward()
            self.a_opt.step()
            if self.nc == 2 and self.num_learn > 0:
                self.soft()
        if self.nc == 1:
            self.soft()
        self.num_learn += 1
        return losses


def cpu_updates(threads):
    torch.set_num_threads(threads)
    # the update, checked against the reference's record before it is timed
    z = np.load(os.path.join(ROOT, "tests", "golden", "td3.npz"))
    chk = CpuAgent(int(z["hyper/S"]), int(z["hyper/A"]), int(z["hyper/H"]), 2, 1e-3, 1e-3)
    for net, name in [(chk.actor, "actor"), (chk.t_actor, "target_actor")] + [(c, f"critic{i + 1}") for i, c in enumerate(chk.critics)] + \
                     [(c, f"target_critic{i + 1}") for i, c in enumerate(chk.t_critics)]:
        net.load_state_dict({k: torch.from_numpy(z[f"sd0/{name}/{k}"]) for k in net.state_dict()})
    t = lambda k: torch.from_numpy(z[f"r1/learn/{k}"]).float()
    losses = chk.learn(t("state"), t("action"), t("reward"), t("next_state"), t("done"), eps=t("eps"))
    for got, key in zip(losses, ("critic_loss1", "critic_loss2")):
        ref = float(z[f"r1/result/{key}"])
        assert abs(got - ref) <= 1e-5 * abs(ref), f"CPU update does not reproduce the fixture: {key} {got!r} vs {ref!r}"
    out = {}
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(B, S, generator=g), torch.tanh(torch.randn(B, A, generator=g)), torch.randn(B, 1, generator=g), torch.randn(B, S, generator=g),
             (torch.rand(B, 1, generator=g) < 0.02).float())
    for name, nc in (("td3", 2), ("ddpg", 1)):
        ag = CpuAgent(S, A, H, nc, OPT[name]["actor_lr"], OPT[name]["critic_lr"])
        for _ in range(4):
            ag.learn(*batch)
        n = 40
        t0 = time.perf_counter()
        for _ in range(n):
            ag.learn(*batch)
        s = (time.perf_counter() - t0) / n
        out[name] = {"update_ms": round(s * 1e3, 3), "updates_per_s": round(1.0 / s, 1)}
    out.update(threads=threads, checked_against="tests/golden/td3.npz record r1 (critic losses to 1e-5)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations td3 / ddpg; the median is reported")
    ap.add_argument("--cpu", action="store_true", help="also time the same updates in torch on the CPU")
    ap.add_argument("--cpu-threads", type=int, default=8)
    args = ap.parse_args()
    out = {"tool": "tools/bench_td3.py", "shape": "config.td3.mujoco (S 11, A 3, H 512, B 128)", "updates": args.updates, "steps": args.steps, "rounds": args.rounds}
    if torch.cuda.is_available():
        out["device"] = torch.cuda.get_device_name(0)
        torch.manual_seed(0)
        np.random.seed(0)
        agents = {name: make_agent(name) for name in ("td3", "ddpg")}
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
                         "learn_ms_rounds": [round(v * 1e3, 4) for v in learn[name]], "hipgraphs": len(agent._graphs)}
    else:
        out["device"] = None
    if args.cpu:
        out["cpu_torch_update"] = cpu_updates(args.cpu_threads)
    line = json.dumps(out)
    assert len(line) < 6000
    print(line)


if __name__ == "__main__":
    main()
