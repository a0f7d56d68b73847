#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of TD3 and DDPG, from the UNMODIFIED reference agents (core/agent/td3.py, core/agent/ddpg.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  The reference is staged exactly as oracle/gen_golden.py stages it (scratch copy, no bytecode, one torch thread
for the fixtures) and `learn()` runs under gen_golden's line tap; this file holds none of the reference's code.

  tests/golden/td3.npz            S 4, A 3, H 32, B 32, perturbed online and target weights: every tensor stored in full
  tests/golden/td3_odd.npz        S 3, A 1, H 64, B 7
  tests/golden/td3_cartpole.npz   config.td3.cartpole exactly (S 4, A 1, H 256, B 128, lr 1e-3 both, tau 1e-3): recipe weights, thinned
  tests/golden/ddpg.npz           S 4, A 3, H 32, B 32
  tests/golden/ddpg_pendulum.npz  config.ddpg.pendulum exactly (S 3, A 1, H 512, B 128, lr 5e-4 / 1e-3, tau 1e-3): recipe weights, thinned
  tests/golden/curves_reference_td3.json   both agents in the single-mode loop on the control env (CURVE_CONFIG)

A TD3 fixture holds THREE independent single learn() records r0 / r1 / r2 from the same starting state, taken with agent.num_learn set to
0, 1 and 2 beforehand: actor step without soft update, critics only, actor step with soft update.  A DDPG fixture holds one record r0.
Every fixture also holds the initial weights of a freshly constructed reference agent under torch.manual_seed(init_seed), thinned.
hyper/thin_limit > 0: arrays larger than that are synth.thin(v, limit) samples (td3_odd: 1024, the config fixtures: 8192); a network that a
learn() left bit-unchanged is recorded as r<i>/unchanged/<net> = 1 instead of a copy of its weights.

Usage:  python tools/gen_golden_td3.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import argparse
import copy
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import synth  # noqa: E402
from oracle.gen_golden import RECIPE_SEED, LineTap, flat, sd_to_np  # noqa: E402

SPECS = {
    "td3": dict(agent="td3", state_size=4, action_size=3, hidden_size=32, batch_size=32, actor_lr=1e-3, critic_lr=1e-3, tau=5e-3, recipe=False, thin_limit=0),
    "td3_odd": dict(agent="td3", state_size=3, action_size=1, hidden_size=64, batch_size=7, actor_lr=5e-4, critic_lr=1e-3, tau=5e-3, recipe=False, thin_limit=1024),
    "td3_cartpole": dict(agent="td3", state_size=4, action_size=1, hidden_size=256, batch_size=128, actor_lr=1e-3, critic_lr=1e-3, tau=1e-3, recipe=True, thin_limit=8192),
    "ddpg": dict(agent="ddpg", state_size=4, action_size=3, hidden_size=32, batch_size=32, actor_lr=5e-4, critic_lr=1e-3, tau=5e-3, recipe=False, thin_limit=0),
    "ddpg_pendulum": dict(agent="ddpg", state_size=3, action_size=1, hidden_size=512, batch_size=128, actor_lr=5e-4, critic_lr=1e-3, tau=1e-3, recipe=True, thin_limit=8192),
}
NETS = {"td3": ("actor", "target_actor", "critic1", "target_critic1", "critic2", "target_critic2"),  # recipe seed RECIPE_SEED + position
        "ddpg": ("actor", "target_actor", "critic", "target_critic")}
OPTS = {"td3": (("actor", "actor_optimizer"), ("critic1", "critic_optimizer1"), ("critic2", "critic_optimizer2")),
        "ddpg": (("actor", "actor_optimizer"), ("critic", "critic_optimizer"))}
FILL, FILL_SEED, INIT_SEED, NP_SEED, TORCH_SEED = 200, 17, 5, 42, 42
BATCH_KEYS = ["state", "action", "reward", "next_state", "done"]

CURVE_SEEDS = (1, 2, 3)
CURVE_CONFIG = dict(S=11, A=3, steps=8000, chunk=1000, run_step=10000, hidden=256, batch=128, buffer=50000, start=1000, tau=5e-3, gamma=0.99, lr_decay=True,
                    td3=dict(initial_random_step=1000, actor_lr=1e-3, critic_lr=1e-3), ddpg=dict())


def fill_transitions(n, S, A, seed):
    """n synthetic continuous-control transitions (also what the tests store into the HIP agent's buffer: the fixture keeps them as buf_*)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        out.append({"state": rng.randn(1, S).astype(np.float32), "action": np.tanh(rng.randn(1, A)).astype(np.float32),
                    "reward": rng.choice([-1.0, 0.0, 1.0, 0.5], size=(1, 1)), "next_state": rng.randn(1, S).astype(np.float32),
                    "done": np.asarray([[rng.rand() < 0.1]])})
    return out


def _agent_class(kind):
    if kind == "td3":
        from core.agent.td3 import TD3

        return TD3
    from core.agent.ddpg import DDPG

    return DDPG


def record_learn(agent, kind, B, A, num_learn):
    """One learn() of (a copy of) the reference agent under the line tap -> flat dict of everything the tests compare."""
    import torch

    cls = type(agent)
    agent.num_learn = num_learn
    c1 = "critic1" if kind == "td3" else "critic"
    loss1 = "critic_loss1 = F.mse_loss" if kind == "td3" else "critic_loss = F.mse_loss"
    step1 = "self.critic_optimizer1.step()" if kind == "td3" else "self.critic_optimizer.step()"
    markers = {"target": (loss1, BATCH_KEYS + ["noise", "next_action", "target_q"]), "cstep1": (step1, []),
               "actor": ("self.actor_optimizer.zero_grad()", ["action_pred", "actor_loss"]), "astep": ("self.actor_optimizer.step()", [])}
    if kind == "td3":
        markers["cstep2"] = ("self.critic_optimizer2.step()", [])
    tap = LineTap(cls.learn, markers)
    extra, grads = {}, {}

    def on_target(frame):
        loc = frame.f_locals
        with torch.no_grad():
            extra["q1"] = getattr(agent, c1)(loc["state"], loc["action"]).numpy().copy()
            if kind == "td3":
                extra["q2"] = agent.critic2(loc["state"], loc["action"]).numpy().copy()

    def grab(net):
        return lambda frame: grads.update({f"{net}/{k}": p.grad.detach().numpy().copy() for k, p in getattr(agent, net).named_parameters()})

    tap.on_line["target"], tap.on_line["cstep1"], tap.on_line["astep"] = on_target, grab(c1), grab("actor")
    if kind == "td3":
        tap.on_line["cstep2"] = grab("critic2")
    np.random.seed(NP_SEED)
    torch.manual_seed(TORCH_SEED)
    with tap:
        result = agent.learn()
    rec = dict(tap.records["target"][0])
    rec.update(extra)
    if "actor" in tap.records:
        rec.update(tap.records["actor"][0])
    if kind == "td3":  # the raw standard normals behind `noise` (td3.py:159: the first draw from torch's generator inside learn())
        torch.manual_seed(TORCH_SEED)
        eps = torch.randn(B, A)
        assert np.array_equal((eps * agent.target_noise_std).clamp(-agent.target_noise_clip, agent.target_noise_clip).numpy(), rec["noise"])
        rec["eps"] = eps.numpy().copy()
    return rec, grads, {k: np.asarray(v) for k, v in result.items()}


def gen_fixture(name, out_dir):
    import torch

    spec = dict(SPECS[name])
    kind, recipe, limit = spec.pop("agent"), spec.pop("recipe"), spec.pop("thin_limit")
    S, A, H, B = spec["state_size"], spec["action_size"], spec["hidden_size"], spec["batch_size"]
    kw = dict(state_size=S, action_size=A, hidden_size=H, batch_size=B, gamma=0.99, buffer_size=256, start_train_step=0, tau=spec["tau"], run_step=100000, device="cpu",
              optim_config={"actor": "adam", "critic": "adam", "actor_lr": spec["actor_lr"], "critic_lr": spec["critic_lr"]})
    cls = _agent_class(kind)
    out = {}
    # the initial weights of a fresh agent under a recorded seed (construction order, orthogonal_init gains)
    torch.manual_seed(INIT_SEED)
    fresh = cls(**kw)
    for net in NETS[kind]:
        flat(f"init_thin/{net}/", {k: synth.thin(v) for k, v in sd_to_np(getattr(fresh, net).state_dict()).items()}, out)
    torch.manual_seed(3)
    np.random.seed(3)
    agent = cls(**kw)
    with torch.no_grad():
        for i, net in enumerate(NETS[kind]):
            mod = getattr(agent, net)
            if recipe:
                rec = synth.recipe_state_dict({k: v.shape for k, v in mod.state_dict().items()}, RECIPE_SEED + i)
                for k, p in mod.named_parameters():
                    p.copy_(torch.from_numpy(rec[k]))
            else:  # independent draws: every target differs from its online net
                for p in mod.parameters():
                    p.add_(0.1 * torch.randn_like(p))
    agent.memory.first_store = False
    agent.memory.store(fill_transitions(FILL, S, A, FILL_SEED))
    n = agent.memory.size
    for k in agent.memory.buffer[0].keys():
        out[f"buf_{k}"] = np.concatenate([agent.memory.buffer[i][k] for i in range(n)], 0)
    # thin_limit > 0: arrays larger than that are stored as synth.thin(v, limit) samples.  The starting weights of a fixture WITHOUT recipe
    # weights cannot be regenerated and are always stored in full.
    keep = (lambda v: synth.thin(v, limit)) if limit else (lambda v: v)
    keep0 = keep if recipe else (lambda v: v)
    sd0 = {net: sd_to_np(getattr(agent, net).state_dict()) for net in NETS[kind]}
    for net in NETS[kind]:
        flat(f"sd0/{net}/", {k: keep0(v) for k, v in sd0[net].items()}, out)
    for r, num_learn in enumerate((0, 1, 2) if kind == "td3" else (0,)):
        a = copy.deepcopy(agent)
        rec, grads, result = record_learn(a, kind, B, A, num_learn)
        flat(f"r{r}/learn/", rec, out)
        flat(f"r{r}/result/", result, out)
        flat(f"r{r}/grad/", {k: keep(v) for k, v in grads.items()}, out)
        for k, v in grads.items():
            out[f"r{r}/grad_absmax/{k}"] = np.abs(v).max()
        for net in NETS[kind]:  # a network that learn() left bit-unchanged is stored as that statement, not as a copy
            sd1 = sd_to_np(getattr(a, net).state_dict())
            same = all(np.array_equal(sd1[k], sd0[net][k]) for k in sd1)
            out[f"r{r}/unchanged/{net}"] = np.asarray(int(same))
            if not same:
                flat(f"r{r}/sd1/{net}/", {k: keep(v) for k, v in sd1.items()}, out)
        for net, oname in OPTS[kind]:
            opt = getattr(a, oname)
            for k, p in getattr(a, net).named_parameters():
                st = opt.state.get(p)
                if st:
                    out[f"r{r}/opt/{net}/exp_avg/{k}"] = keep(st["exp_avg"].detach().numpy())
                    out[f"r{r}/opt/{net}/exp_avg_sq/{k}"] = keep(st["exp_avg_sq"].detach().numpy())
        out[f"r{r}/num_learn"] = np.asarray(num_learn)
        print(name, f"num_learn={num_learn}", {k: float(v) for k, v in result.items()})
    hyper = dict(gamma=0.99, actor_lr=spec["actor_lr"], critic_lr=spec["critic_lr"], tau=spec["tau"], B=B, S=S, A=A, H=H, np_seed=NP_SEED, torch_seed=TORCH_SEED,
                 init_seed=INIT_SEED, fill=FILL, fill_seed=FILL_SEED, recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit)
    if kind == "td3":
        hyper.update(target_noise_std=agent.target_noise_std, target_noise_clip=agent.target_noise_clip, update_delay=agent.update_delay)
    for k, v in hyper.items():
        out[f"hyper/{k}"] = np.asarray(v)
    out["hyper/agent"] = np.asarray(kind)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, f"{os.path.getsize(path)} bytes")


def curve_agent_kwargs(kind):
    """The keyword arguments of both sides of the curve comparison (tests/test_td3_gpu.py builds the HIP agent from the same function's twin)."""
    c = CURVE_CONFIG
    kw = dict(state_size=c["S"], action_size=c["A"], hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"],
              run_step=c["run_step"], tau=c["tau"], gamma=c["gamma"], lr_decay=c["lr_decay"])
    if kind == "td3":
        t = c["td3"]
        kw.update(initial_random_step=t["initial_random_step"], optim_config={"actor": "adam", "critic": "adam", "actor_lr": t["actor_lr"], "critic_lr": t["critic_lr"]})
    return kw


def control_curve(agent, env, steps, chunk):
    """The single-mode loop (act, step, process([transition], step)) -> mean reward per `chunk` env steps."""
    out, acc = [], []
    state = env.obs()
    for step in range(1, steps + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"], dtype=np.float32).reshape(1, -1))
        tr = {"state": state, "next_state": np.asarray(nxt, dtype=np.float32), "reward": np.asarray(rew, dtype=np.float64).reshape(1, 1),
              "done": np.asarray(done).astype(bool).reshape(1, 1)}
        tr.update(a)
        agent.process([tr], step)
        state = env.obs()
        acc.append(float(np.asarray(rew).reshape(-1)[0]))
        if step % chunk == 0:
            out.append(float(np.mean(acc)))
            acc = []
    return out


def reference_curve(kind, seed):
    import torch

    from oracle.jorldy_oracle import ControlOracle

    c = CURVE_CONFIG
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = _agent_class(kind)(device="cpu", **curve_agent_kwargs(kind))
    agent.memory.first_store = False
    return control_curve(agent, ControlOracle(1, c["S"], c["A"], seed=1000 + seed), c["steps"], c["chunk"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (the directory that holds jorldy/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="fixtures,curves")
    ap.add_argument("--threads", type=int, default=4, help="torch threads of the curve runs (the fixtures always use one)")
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    os.makedirs(out_dir, exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="jref_")
    subprocess.check_call(f"cd {args.ref} && tar --exclude='jorldy/core/env/mlagents' -cf - jorldy | (cd {scratch} && tar xf -)", shell=True)
    cwd = os.getcwd()
    os.chdir(os.path.join(scratch, "jorldy"))
    sys.path.insert(0, os.getcwd())
    sys.dont_write_bytecode = True
    import torch

    try:
        todo = args.only.split(",")
        if "fixtures" in todo:
            torch.set_num_threads(1)  # deterministic reductions in the fixtures
            for name in SPECS:
                gen_fixture(name, out_dir)
        if "curves" in todo:
            torch.set_num_threads(args.threads)
            doc = {"generator": "tools/gen_golden_td3.py --only curves (the unmodified reference TD3 / DDPG, CPU, scratch copy)", "seeds": list(CURVE_SEEDS),
                   "torch_threads": args.threads, "config": CURVE_CONFIG, "metric": "mean reward per 1000 env steps"}
            for kind in ("td3", "ddpg"):
                curves = []
                for s in CURVE_SEEDS:
                    curves.append(reference_curve(kind, s))
                    print(kind, "curve seed", s, [round(v, 3) for v in curves[-1]], flush=True)
                doc[kind] = {"reference": curves}
            with open(os.path.join(out_dir, "curves_reference_td3.json"), "w") as f:
                json.dump(doc, f, indent=1)
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    print("written to", out_dir)


if __name__ == "__main__":
    main()
