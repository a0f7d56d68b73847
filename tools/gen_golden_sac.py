#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of the continuous SAC, from the UNMODIFIED reference agent (core/agent/sac.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs and the actor-critic family's starting point, record layout and curve
loop are oracle/refkit.py's; this file holds none of the reference's code.

  tests/golden/sac.npz            S 4, A 3, H 32, B 32, dynamic alpha with alpha_lr 5e-2 (one alpha step is visible), perturbed online and
                                  target weights, every tensor stored in full; TWO CONSECUTIVE learns r0 and r1 -- r1 starts where r0 ended,
                                  which pins the one-step lag of alpha
  tests/golden/sac_odd.npz        S 3, A 1, H 64, B 7, static alpha (static_log_alpha -2.0), one record
  tests/golden/sac_pendulum.npz   config.sac.pendulum exactly (S 3, A 1, H 512, B 64, lr 5e-4 / 1e-3 / 3e-4, tau 5e-3, dynamic): recipe weights,
                                  thinned, one record
  tests/golden/curves_reference_sac.json   the agent in the single-mode loop on the control env (CURVE_CONFIG)

A record holds the batch, both normal draws (the target's, the actor step's), a', logp', y, q1, q2, the actor step's a, logp, q_i and min_q,
the result keys, the gradients, Adam moments and end weights of every network, log_alpha, alpha and the alpha optimizer's moments before and
after.  Every fixture also holds the initial weights of a freshly constructed reference agent under torch.manual_seed(init_seed), thinned.
The actor's mu / log_std matrices are scaled by hyper/head_scale after the perturbation / the recipe.  hyper/thin_limit > 0: arrays larger than that are synth.thin(v, limit) samples; a network that a learn() left bit-unchanged is recorded as
r<i>/unchanged/<net> = 1 instead of a copy of its weights.

Usage:  python tools/gen_golden_sac.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED, LineTap, flat, sd_to_np  # noqa: E402

SPECS = {
    "sac": dict(state_size=4, action_size=3, hidden_size=32, batch_size=32, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=5e-2, tau=5e-3, dynamic=True, records=2,
                recipe=False, thin_limit=0),
    "sac_odd": dict(state_size=3, action_size=1, hidden_size=64, batch_size=7, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=3e-4, tau=5e-3, dynamic=False, records=1,
                    recipe=False, thin_limit=1024),
    "sac_pendulum": dict(state_size=3, action_size=1, hidden_size=512, batch_size=64, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=3e-4, tau=5e-3, dynamic=True, records=1,
                         recipe=True, thin_limit=8192),
}
NETS = ("actor", "critic1", "target_critic1", "critic2", "target_critic2")  # the reference's construction order; recipe seed RECIPE_SEED + position
OPTS = (("actor", "actor_optimizer"), ("critic1", "critic_optimizer1"), ("critic2", "critic_optimizer2"))
FILL, INIT_SEED, NP_SEED, TORCH_SEED, PERTURB, STATIC_LOG_ALPHA = 200, 5, 42, 42, 0.05, -2.0
HEAD_SCALE = 0.2  # the actor's mu / log_std matrices are scaled down (as synth.ppo_recipe does) so that the fixtures' samples stay clear of tanh's saturation
BATCH_KEYS = ["state", "action", "reward", "next_state", "done"]

CURVE_SEEDS = (1, 2, 3)
CURVE_CONFIG = dict(S=11, A=3, steps=12000, chunk=1000, run_step=15000, hidden=256, batch=128, buffer=50000, start=1000, tau=5e-3, gamma=0.99, lr_decay=True,
                    sac=dict(use_dynamic_alpha=True, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=3e-4),
                    note="12000 steps, not TD3's 8000: over 8000 the reference's own three seeds rise by 0.27, short of the 0.3 that 'learns' asks for")


def _alpha_state(agent):
    import torch

    out = {"log_alpha": np.asarray(float(agent.log_alpha.detach().reshape(-1)[0]), np.float32), "alpha": np.asarray(float(agent.alpha.detach().reshape(-1)[0]), np.float32)}
    st = agent.alpha_optimizer.state.get(agent.log_alpha) if agent.alpha_optimizer is not None else None
    out["step"] = np.asarray(int(float(st["step"])) if st else 0)
    out["exp_avg"] = np.asarray(float(st["exp_avg"]) if st else 0.0, np.float32)
    out["exp_avg_sq"] = np.asarray(float(st["exp_avg_sq"]) if st else 0.0, np.float32)
    assert torch.is_tensor(agent.log_alpha)
    return out


def record_learn(agent, B, A, np_seed, torch_seed):
    """One learn() of the reference agent (IN PLACE) under the line tap -> flat dict of everything the tests compare."""
    import torch

    cls = type(agent)
    markers = {"target": ("critic_loss1 = F.mse_loss", BATCH_KEYS + ["q1", "q2", "next_action", "next_log_prob", "target_q"]),
               "cstep1": ("self.critic_optimizer1.step()", []), "cstep2": ("self.critic_optimizer2.step()", []),
               "actor": ("self.actor_optimizer.zero_grad", ["sample_action", "log_prob", "min_q", "actor_loss"]), "astep": ("self.actor_optimizer.step()", [])}
    tap = LineTap(cls.learn, markers)
    extra, grads = {}, {}

    def on_actor(frame):
        loc = frame.f_locals
        extra["q1_pi"], extra["q2_pi"] = loc["q1"].detach().numpy().copy(), loc["q2"].detach().numpy().copy()

    def grab(net):
        return lambda frame: grads.update({f"{net}/{k}": g for k, g in refkit.grads_of(getattr(agent, net)).items()})

    tap.on_line["actor"], tap.on_line["cstep1"], tap.on_line["cstep2"], tap.on_line["astep"] = on_actor, grab("critic1"), grab("critic2"), grab("actor")
    before = copy.deepcopy(agent.actor)
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    with tap:
        result = agent.learn()
    rec = dict(tap.records["target"][0])
    rec.update(tap.records["actor"][0])
    rec.update(extra)
    # the raw standard normals behind the two samples: the first two [B, A] draws from torch's generator inside learn()
    torch.manual_seed(torch_seed)
    eps_t, eps_a = torch.randn(B, A), torch.randn(B, A)
    with torch.no_grad():
        mu, std = before(torch.as_tensor(rec["next_state"]))
        assert np.array_equal(torch.tanh(mu + eps_t * std).numpy(), rec["next_action"]), "the target's draw is not the generator's first"
        mu, std = before(torch.as_tensor(rec["state"]))
        assert np.array_equal(torch.tanh(mu + eps_a * std).numpy(), rec["sample_action"]), "the actor step's draw is not the generator's second"
    rec["eps_target"], rec["eps_actor"] = eps_t.numpy().copy(), eps_a.numpy().copy()
    return rec, grads, {k: np.asarray(v) for k, v in result.items()}


def agent_kwargs(spec):
    return dict(state_size=spec["state_size"], action_size=spec["action_size"], hidden_size=spec["hidden_size"], batch_size=spec["batch_size"], gamma=0.99,
                buffer_size=256, start_train_step=0, tau=spec["tau"], run_step=100000, device="cpu", use_dynamic_alpha=spec["dynamic"], static_log_alpha=STATIC_LOG_ALPHA,
                optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": spec["actor_lr"], "critic_lr": spec["critic_lr"], "alpha_lr": spec["alpha_lr"]})


def scale_heads(agent):
    for layer in (agent.actor.mu, agent.actor.log_std):
        layer.weight.mul_(float(np.float32(HEAD_SCALE)))


def gen_fixture(name, out_dir):
    from core.agent.sac import SAC

    spec = dict(SPECS[name])
    recipe, limit = spec["recipe"], spec["thin_limit"]
    S, A, H, B = spec["state_size"], spec["action_size"], spec["hidden_size"], spec["batch_size"]
    out = {}
    agent, _, keep = refkit.actor_critic_agent(SAC, agent_kwargs(spec), NETS, out, recipe, PERTURB, limit, INIT_SEED, FILL, tweak=scale_heads)
    for r in range(spec["records"]):  # consecutive: record r + 1 starts where record r ended
        start = {net: sd_to_np(getattr(agent, net).state_dict()) for net in NETS}
        flat(f"r{r}/alpha0/", _alpha_state(agent), out)
        rec, grads, result = record_learn(agent, B, A, NP_SEED + r, TORCH_SEED + r)
        alpha1 = {f"alpha1/{k}": v for k, v in _alpha_state(agent).items()}
        refkit.store_actor_critic_record(out, r, agent, NETS, OPTS, start, rec, grads, result, keep, then=alpha1)
        out[f"r{r}/np_seed"], out[f"r{r}/torch_seed"] = np.asarray(NP_SEED + r), np.asarray(TORCH_SEED + r)
        sat = float(1 - np.abs(np.concatenate([rec["next_action"].reshape(-1), rec["sample_action"].reshape(-1)])).max() ** 2)
        print(name, f"r{r}", {k: float(v) for k, v in result.items()}, f"min 1 - a^2 = {sat:.3e}")
    hyper = dict(gamma=0.99, actor_lr=spec["actor_lr"], critic_lr=spec["critic_lr"], alpha_lr=spec["alpha_lr"], tau=spec["tau"], B=B, S=S, A=A, H=H, init_seed=INIT_SEED,
                 fill=FILL, fill_seed=FILL_SEED, recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit, use_dynamic_alpha=int(spec["dynamic"]),
                 static_log_alpha=STATIC_LOG_ALPHA, target_entropy=float(agent.target_entropy), perturb=PERTURB, head_scale=HEAD_SCALE, agent="sac")
    refkit.put_hyper(out, hyper)
    refkit.save_fixture(out_dir, name, out)


def curve_agent_kwargs():
    """The keyword arguments of both sides of the curve comparison (tests/test_sac_gpu.py builds the HIP agent from the same function's twin)."""
    c = CURVE_CONFIG
    t = c["sac"]
    return dict(state_size=c["S"], action_size=c["A"], hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"],
                run_step=c["run_step"], tau=c["tau"], gamma=c["gamma"], lr_decay=c["lr_decay"], use_dynamic_alpha=t["use_dynamic_alpha"],
                optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": t["actor_lr"], "critic_lr": t["critic_lr"], "alpha_lr": t["alpha_lr"]})


def reference_curve(seed):
    from core.agent.sac import SAC

    refkit.seed_rngs(seed)
    return refkit.control_oracle_curve(SAC(device="cpu", **curve_agent_kwargs()), seed, CURVE_CONFIG)


def gen_curves(out_dir, threads):
    doc = refkit.curve_doc("tools/gen_golden_sac.py --only curves (the unmodified reference SAC, CPU, scratch copy)", CURVE_SEEDS, threads,
                           config=CURVE_CONFIG, metric="mean reward per 1000 env steps", sac={"reference": refkit.seeded_curves(reference_curve, CURVE_SEEDS, "sac", digits=3)})
    refkit.write_curves(os.path.join(out_dir, "curves_reference_sac.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
