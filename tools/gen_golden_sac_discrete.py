#!/usr/bin/env python3
"""Golden vectors and the reference CartPole curves of the discrete SAC, from the UNMODIFIED reference agent (core/agent/sac.py with
actor discrete_policy, critic discrete_q_network).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or reads the
reference.  Staging, the main, the line tap, the actor-critic family's starting point, record layout and curve loop are oracle/refkit.py's;
this file holds none of the reference's code.

  tests/golden/sac_discrete.npz            S 4, A 3, H 64, B 32, dynamic alpha with alpha_lr 5e-2, perturbed online and target weights, every
                                           tensor in full; THREE CONSECUTIVE learns r0..r2: r1 uses the alpha r0 refreshed (still exp(0)), r2 is
                                           the first whose alpha shows log_alpha's first Adam step -- the one-learn lag
  tests/golden/sac_discrete_static.npz     S 3, A 2, H 32, B 7, static alpha (static_log_alpha -2.0); two learns with a hard target update
                                           between them (r1/target0/ holds the targets r1 starts from)
  tests/golden/sac_discrete_cartpole.npz   config.sac.cartpole_discrete exactly (S 4, A 2, H 512, B 64, lr 1.5e-4 / 3e-4 / 1e-5, dynamic): recipe
                                           weights, thinned, one record
  tests/golden/curves_reference_sac_discrete.json   the agent in the single-mode loop on the oracle's CartPole (CURVE_CONFIG), three seeds

A record holds the batch, pi', next_q_i, H', y, q_i at the taken action, the actor step's pi, q_i, H and min_q, the raw logits of the actor on
s and the critics' Q rows on s with their gradients (head gradients), the result keys, the gradients, Adam moments and end weights of every
network, log_alpha, alpha and the alpha optimizer's moments before and after.  The stored actions are the argmax of refkit's continuous fill
actions, as [1, 1] indices.

Usage:  python tools/gen_golden_sac_discrete.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED, LineTap, flat, sd_to_np  # noqa: E402

SPECS = {
    "sac_discrete": dict(state_size=4, action_size=3, hidden_size=64, batch_size=32, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=5e-2, dynamic=True, records=3,
                         hard_before=(), recipe=False, thin_limit=0),
    "sac_discrete_static": dict(state_size=3, action_size=2, hidden_size=32, batch_size=7, actor_lr=5e-4, critic_lr=1e-3, alpha_lr=3e-4, dynamic=False, records=2,
                                hard_before=(1,), recipe=False, thin_limit=0),
    "sac_discrete_cartpole": dict(state_size=4, action_size=2, hidden_size=512, batch_size=64, actor_lr=1.5e-4, critic_lr=3e-4, alpha_lr=1e-5, dynamic=True, records=1,
                                  hard_before=(), recipe=True, thin_limit=8192),
}
NETS = ("actor", "critic1", "target_critic1", "critic2", "target_critic2")  # the reference's construction order; recipe seed RECIPE_SEED + position
OPTS = (("actor", "actor_optimizer"), ("critic1", "critic_optimizer1"), ("critic2", "critic_optimizer2"))
FILL, INIT_SEED, NP_SEED, TORCH_SEED, PERTURB, STATIC_LOG_ALPHA = 200, 5, 42, 42, 0.05, -2.0
BATCH_KEYS = ["state", "action", "reward", "next_state", "done"]

CURVE_SEEDS = (1, 2, 3)
CURVE_CONFIG = dict(steps=6000, chunk=500, run_step=6000, hidden=128, batch=64, buffer=50000, start=500, gamma=0.99, lr_decay=True, target_update_period=500,
                    sac=dict(use_dynamic_alpha=True, actor_lr=1.5e-4, critic_lr=3e-4, alpha_lr=1e-5),
                    note="config.sac.cartpole_discrete's optimizer and target period at hidden 128, start 500 and 6000 steps: what a test can afford")


def _alpha_state(agent):
    out = {"log_alpha": np.asarray(float(agent.log_alpha.detach().reshape(-1)[0]), np.float32), "alpha": np.asarray(float(agent.alpha.detach().reshape(-1)[0]), np.float32)}
    st = agent.alpha_optimizer.state.get(agent.log_alpha) if agent.alpha_optimizer is not None else None
    out["step"] = np.asarray(int(float(st["step"])) if st else 0)
    out["exp_avg"] = np.asarray(float(st["exp_avg"]) if st else 0.0, np.float32)
    out["exp_avg_sq"] = np.asarray(float(st["exp_avg_sq"]) if st else 0.0, np.float32)
    return out


def record_learn(agent, np_seed, torch_seed):
    """One learn() of the reference agent (IN PLACE) under the line tap -> flat dict of everything the tests compare."""
    import torch

    markers = {"target": ("critic_loss1 = F.mse_loss", BATCH_KEYS + ["q1", "q2", "next_pi", "next_q1", "next_q2", "entropy", "target_q"]),
               "cstep1": ("self.critic_optimizer1.step()", []), "cstep2": ("self.critic_optimizer2.step()", []),
               "actor": ("self.actor_optimizer.zero_grad", ["pi", "q1", "q2", "entropy", "min_q", "actor_loss"]), "astep": ("self.actor_optimizer.step()", [])}
    tap = LineTap(type(agent).learn, markers)
    grads, heads = {}, {}
    outs, hooks = refkit.retaining_hooks({"logits": agent.actor.pi, "q1_all": agent.critic1.q, "q2_all": agent.critic2.q})

    def grab(net, tags):
        def on_line(frame):
            grads.update({f"{net}/{k}": g for k, g in refkit.grads_of(getattr(agent, net)).items()})
            for tag, i in tags:  # the forward whose gradient this step applies: the critics' FIRST (on s), the actor's LAST (on s)
                heads[tag], heads["d_" + tag] = outs[tag][i].detach().numpy().copy(), outs[tag][i].grad.detach().numpy().copy()
        return on_line

    tap.on_line["cstep1"], tap.on_line["cstep2"], tap.on_line["astep"] = grab("critic1", [("q1_all", 0)]), grab("critic2", [("q2_all", 0)]), grab("actor", [("logits", -1)])
    np.random.seed(np_seed)
    torch.manual_seed(torch_seed)
    with tap:
        result = agent.learn()
    for h in hooks:
        h.remove()
    rec = {(k + "_next" if k == "entropy" else k): v for k, v in tap.records["target"][0].items()}
    rec.update({{"q1": "q1_pi", "q2": "q2_pi"}.get(k, k): v for k, v in tap.records["actor"][0].items()})
    rec.update(heads)
    rec["logits_next"] = outs["logits"][0].detach().numpy().copy()  # the actor on s' (under no_grad)
    rec["qt1_next"], rec["qt2_next"] = (getattr(agent, t)(torch.as_tensor(rec["next_state"])).detach().numpy().copy() for t in ("_t1", "_t2"))
    rec["q1_after"], rec["q2_after"] = outs["q1_all"][-1].detach().numpy().copy(), outs["q2_all"][-1].detach().numpy().copy()
    return rec, grads, {k: np.asarray(v) for k, v in result.items()}


def agent_kwargs(spec):
    return dict(state_size=spec["state_size"], action_size=spec["action_size"], hidden_size=spec["hidden_size"], batch_size=spec["batch_size"], gamma=0.99,
                actor="discrete_policy", critic="discrete_q_network", buffer_size=256, start_train_step=0, run_step=100000, device="cpu",
                use_dynamic_alpha=spec["dynamic"], static_log_alpha=STATIC_LOG_ALPHA,
                optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": spec["actor_lr"], "critic_lr": spec["critic_lr"], "alpha_lr": spec["alpha_lr"]})


def index_actions(agent, out):
    """refkit's fill stores continuous [1, A] actions: a discrete agent's buffer holds the index [1, 1] -- the argmax of the same draw."""
    for i in range(agent.memory.size):
        agent.memory.buffer[i]["action"] = np.argmax(agent.memory.buffer[i]["action"], axis=1).reshape(1, 1).astype(np.int64)
    refkit.dump_buffer(agent, out)


def gen_fixture(name, out_dir):
    import copy

    from core.agent.sac import SAC

    spec = dict(SPECS[name])
    recipe, limit = spec["recipe"], spec["thin_limit"]
    out = {}
    agent, _, keep = refkit.actor_critic_agent(SAC, agent_kwargs(spec), NETS, out, recipe, PERTURB, limit, INIT_SEED, FILL)
    index_actions(agent, out)
    for r in range(spec["records"]):  # consecutive: record r + 1 starts where record r ended
        if r in spec["hard_before"]:
            agent.update_target_hard()
            for t in ("target_critic1", "target_critic2"):
                flat(f"r{r}/target0/{t}/", {k: keep(v) for k, v in sd_to_np(getattr(agent, t).state_dict()).items()}, out)
        start = {net: sd_to_np(getattr(agent, net).state_dict()) for net in NETS}
        agent._t1, agent._t2 = copy.deepcopy(agent.target_critic1), copy.deepcopy(agent.target_critic2)  # the targets this learn reads, for qt*_next
        flat(f"r{r}/alpha0/", _alpha_state(agent), out)
        rec, grads, result = record_learn(agent, NP_SEED + r, TORCH_SEED + r)
        alpha1 = {f"alpha1/{k}": v for k, v in _alpha_state(agent).items()}
        refkit.store_actor_critic_record(out, r, agent, NETS, OPTS, start, rec, grads, result, keep, then=alpha1)
        out[f"r{r}/np_seed"], out[f"r{r}/torch_seed"] = np.asarray(NP_SEED + r), np.asarray(TORCH_SEED + r)
        print(name, f"r{r}", {k: float(v) for k, v in result.items()})
    hyper = dict(gamma=0.99, actor_lr=spec["actor_lr"], critic_lr=spec["critic_lr"], alpha_lr=spec["alpha_lr"], B=spec["batch_size"], S=spec["state_size"],
                 A=spec["action_size"], H=spec["hidden_size"], init_seed=INIT_SEED, fill=FILL, fill_seed=FILL_SEED, recipe=int(recipe), recipe_seed=RECIPE_SEED,
                 thin_limit=limit, use_dynamic_alpha=int(spec["dynamic"]), static_log_alpha=STATIC_LOG_ALPHA, target_entropy=float(agent.target_entropy),
                 perturb=PERTURB, records=spec["records"], agent="sac_discrete")
    refkit.put_hyper(out, hyper)
    refkit.save_fixture(out_dir, name, out)


def curve_agent_kwargs():
    """The keyword arguments of both sides of the curve comparison (tools/bench_sac.py's discrete_curve builds the HIP agent from the JSON's config)."""
    c = CURVE_CONFIG
    t = c["sac"]
    return dict(state_size=4, action_size=2, hidden_size=c["hidden"], batch_size=c["batch"], buffer_size=c["buffer"], start_train_step=c["start"], run_step=c["run_step"],
                gamma=c["gamma"], lr_decay=c["lr_decay"], target_update_period=c["target_update_period"], actor="discrete_policy", critic="discrete_q_network",
                use_dynamic_alpha=t["use_dynamic_alpha"],
                optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": t["actor_lr"], "critic_lr": t["critic_lr"], "alpha_lr": t["alpha_lr"]})


def reference_curve(seed):
    from core.agent.sac import SAC

    refkit.seed_rngs(seed)
    agent = SAC(device="cpu", **curve_agent_kwargs())
    agent.memory.first_store = False
    return refkit.value_cartpole_curve(agent, seed, CURVE_CONFIG["steps"], CURVE_CONFIG["chunk"])


def gen_curves(out_dir, threads):
    doc = refkit.curve_doc("tools/gen_golden_sac_discrete.py --only curves (the unmodified reference SAC, discrete, CPU, scratch copy)", CURVE_SEEDS, threads,
                           config=CURVE_CONFIG, metric="mean episode length per 500 env steps",
                           sac_discrete={"reference": refkit.seeded_curves(reference_curve, CURVE_SEEDS, "sac_discrete", digits=1)})
    refkit.write_curves(os.path.join(out_dir, "curves_reference_sac_discrete.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
