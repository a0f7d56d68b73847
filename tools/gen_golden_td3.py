#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of TD3 and DDPG, from the UNMODIFIED reference agents (core/agent/td3.py, core/agent/ddpg.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs and the actor-critic family's starting point, record layout and curve
loop are oracle/refkit.py's; this file holds none of the reference's code.

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
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED, LineTap  # noqa: E402

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
FILL, INIT_SEED, NP_SEED, TORCH_SEED = 200, 5, 42, 42
BATCH_KEYS = ["state", "action", "reward", "next_state", "done"]

CURVE_SEEDS = (1, 2, 3)
CURVE_CONFIG = dict(S=11, A=3, steps=8000, chunk=1000, run_step=10000, hidden=256, batch=128, buffer=50000, start=1000, tau=5e-3, gamma=0.99, lr_decay=True,
                    td3=dict(initial_random_step=1000, actor_lr=1e-3, critic_lr=1e-3), ddpg=dict())


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
        return lambda frame: grads.update({f"{net}/{k}": g for k, g in refkit.grads_of(getattr(agent, net)).items()})

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
    spec = dict(SPECS[name])
    kind, recipe, limit = spec.pop("agent"), spec.pop("recipe"), spec.pop("thin_limit")
    S, A, H, B = spec["state_size"], spec["action_size"], spec["hidden_size"], spec["batch_size"]
    kw = dict(state_size=S, action_size=A, hidden_size=H, batch_size=B, gamma=0.99, buffer_size=256, start_train_step=0, tau=spec["tau"], run_step=100000, device="cpu",
              optim_config={"actor": "adam", "critic": "adam", "actor_lr": spec["actor_lr"], "critic_lr": spec["critic_lr"]})
    out = {}
    agent, sd0, keep = refkit.actor_critic_agent(_agent_class(kind), kw, NETS[kind], out, recipe, 0.1, limit, INIT_SEED, FILL)
    for r, num_learn in enumerate((0, 1, 2) if kind == "td3" else (0,)):  # independent records: each from a copy of the same starting state
        a = copy.deepcopy(agent)
        rec, grads, result = record_learn(a, kind, B, A, num_learn)
        refkit.store_actor_critic_record(out, r, a, NETS[kind], OPTS[kind], sd0, rec, grads, result, keep)
        out[f"r{r}/num_learn"] = np.asarray(num_learn)
        print(name, f"num_learn={num_learn}", {k: float(v) for k, v in result.items()})
    hyper = dict(gamma=0.99, actor_lr=spec["actor_lr"], critic_lr=spec["critic_lr"], tau=spec["tau"], B=B, S=S, A=A, H=H, np_seed=NP_SEED, torch_seed=TORCH_SEED,
                 init_seed=INIT_SEED, fill=FILL, fill_seed=FILL_SEED, recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit)
    if kind == "td3":
        hyper.update(target_noise_std=agent.target_noise_std, target_noise_clip=agent.target_noise_clip, update_delay=agent.update_delay)
    refkit.put_hyper(out, dict(hyper, agent=kind))
    refkit.save_fixture(out_dir, name, out)


def curve_agent_kwargs(kind):
    """The keyword arguments of both sides of the curve comparison (tests/test_td3_gpu.py builds the HIP agent from the same function's twin)."""
    c = CURVE_CONFIG
    kw = dict(state_size=c["S"], action_size=c["A"], hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"],
              run_step=c["run_step"], tau=c["tau"], gamma=c["gamma"], lr_decay=c["lr_decay"])
    if kind == "td3":
        t = c["td3"]
        kw.update(initial_random_step=t["initial_random_step"], optim_config={"actor": "adam", "critic": "adam", "actor_lr": t["actor_lr"], "critic_lr": t["critic_lr"]})
    return kw


def reference_curve(kind, seed):
    refkit.seed_rngs(seed)
    return refkit.control_oracle_curve(_agent_class(kind)(device="cpu", **curve_agent_kwargs(kind)), seed, CURVE_CONFIG)


def gen_curves(out_dir, threads):
    doc = refkit.curve_doc("tools/gen_golden_td3.py --only curves (the unmodified reference TD3 / DDPG, CPU, scratch copy)", CURVE_SEEDS, threads,
                           config=CURVE_CONFIG, metric="mean reward per 1000 env steps")
    for kind in ("td3", "ddpg"):
        doc[kind] = {"reference": refkit.seeded_curves(lambda s: reference_curve(kind, s), CURVE_SEEDS, kind, digits=3)}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_td3.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
