#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of discrete MPO, from the UNMODIFIED reference agent (core/agent/mpo.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs, the hooks, the storage helpers and the on-policy curve loop are
oracle/refkit.py's; this file holds none of the reference's code.

  tests/golden/mpo_discrete.npz   S 4, A 3, H 32, B 5 trajectories of T 4 (R 20) out of 12 stored, Retrace.  Multipliers 2.0 / 0.1 / 1.0, lr 3e-3 (one
                                  multiplier step is visible), perturbed weights (the targets a little away from their online nets), every tensor in
                                  full; TWO CONSECUTIVE learns l0, l1, then update_target
  tests/golden/mpo_td.npz         the same with critic_loss_type '1step_TD' (T 1), A 2, one learn; min_eta = 0.999 under eta = 1: the first step (a
                                  positive gradient, a step of lr down) crosses the floor and is clamped
  tests/golden/mpo_cartpole.npz   config.mpo.cartpole exactly (H 512, B 64, T 4, lr 2.5e-4, 1.0 / 1.0 / 1.0, eps 0.02 / 0.01 / 0.01): recipe weights and a
                                  recipe replay (regenerated from seeds by the reader), big arrays thinned, one learn
  tests/golden/curves_reference_mpo.json   the oracle's CartPole in single mode, tests/mpo_truth.py's CURVE_CONFIG, seeds 1-3: mean reward per step
                                  in bins of 100 steps

A learn `l<k>/` holds the sampled rows `idx`, the six network outputs (actor logits la, la_next, la_old and critic q, qt, qt_next), c, Qret before
(`qret0`) and after (`qret`) the Retrace scan, At, the E-step weights, the four losses, d(loss)/d la and d(loss)/d q, the multipliers with their
gradients and Adam moments before and after the step, both nets' parameter gradients raw and clipped, their end weights `sd1/`, and `result/`.
hyper/thin_limit > 0: arrays larger than that are strided samples (tests/mpo_truth.py's thin).
Conditions the generator asserts on the SAMPLED batch (the replay seed is the first from 5 up that meets them): done = 1 inside at least two
trajectories, one of them at position T - 2 (Retrace fixtures); c clipped in some rows and unclipped in others.

Usage:  python tools/gen_golden_mpo.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpo_truth as D  # noqa: E402  (the replay recipe, the recipe weights and the curve configuration are shared with the tests)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import RECIPE_SEED, LineTap, flat, grads_of, sd_to_np  # noqa: E402

SPECS = {
    "mpo_discrete": dict(S=4, A=3, H=32, B=5, T=4, N=12, retrace=True, lr=3e-3, mult=(2.0, 0.1, 1.0), floors=(1e-8, 1e-8, 1e-8), eps=(0.01, 0.01, 5e-5), learns=2,
                         recipe=False, thin_limit=0),
    "mpo_td": dict(S=4, A=2, H=32, B=5, T=1, N=12, retrace=False, lr=3e-3, mult=(1.0, 0.1, 1.0), floors=(0.999, 1e-8, 1e-8), eps=(0.1, 0.01, 5e-5), learns=1,
                   recipe=False, thin_limit=0),
    "mpo_cartpole": dict(S=4, A=2, H=512, B=64, T=4, N=300, retrace=True, lr=2.5e-4, mult=(1.0, 1.0, 1.0), floors=(1e-8, 1e-8, 1e-8), eps=(0.02, 0.01, 0.01), learns=1,
                         recipe=True, thin_limit=8192),
}
GAMMA, CLIP, INIT_SEED, NP_SEED, PERTURB, PERTURB_TARGET = 0.99, 1.0, 11, 21, 0.05, 0.02
BIN = 100


def agent_kwargs(spec):
    kw = dict(state_size=spec["S"], action_size=spec["A"], hidden_size=spec["H"], actor="discrete_policy", critic="discrete_q_network",
              optim_config={"name": "adam", "lr": spec["lr"]}, gamma=GAMMA, buffer_size=max(spec["N"], 64), batch_size=spec["B"], start_train_step=0, n_epoch=spec["learns"],
              n_step=spec["T"] if spec["retrace"] else 8, clip_grad_norm=CLIP, run_step=100000, lr_decay=False, device="cpu",
              critic_loss_type="retrace" if spec["retrace"] else "1step_TD")
    for j, k in enumerate(D.NAMES):
        kw[k], kw["min_" + k], kw["eps_" + k] = spec["mult"][j], spec["floors"][j], spec["eps"][j]
    return kw


def multiplier_state(agent):
    return refkit.multiplier_state(agent, D.NAMES, agent.actor_optimizer)


def record_learn(agent, spec, keep):
    """One learn() of the reference agent (IN PLACE) under the line tap -> flat dict."""
    outs, hooks = refkit.retaining_hooks({"actor": agent.actor.pi, "target_actor": agent.target_actor.pi, "critic": agent.critic.q, "target_critic": agent.target_critic.q})
    markers = {
        "scan": ("reversed(\n", ["Qret"]),  # the discrete branch's loop header (the continuous branch writes it on one line): first hit = before the scan
        "target": ("critic_loss = F.mse_loss(Q_a, Qret)", ["Qret", "c", "action", "reward", "prob_b", "state", "next_state"]),
        "loss": ("loss = critic_loss + actor_loss", ["At", "q", "KLD_pi", "actor_loss", "critic_loss", "eta_loss", "alpha_loss"]),
        "grad": ("torch.nn.utils.clip_grad_norm_(self.actor.parameters()", []),
        "step": ("self.actor_optimizer.step()", []),
        "after": ("self.num_learn += 1", []),
    }
    tap = LineTap(type(agent).learn, markers)
    nets = {"actor": agent.actor, "critic": agent.critic}
    got = {}

    def on_grad(frame):
        got["raw"] = {n: grads_of(net) for n, net in nets.items()}
        got["d_la"], got["d_q"] = outs["actor"][0].grad.detach().numpy().copy(), outs["critic"][0].grad.detach().numpy().copy()
        assert outs["actor"][1].grad is None, "online(s') carries no gradient"
        got["mult_grad"] = refkit.multiplier_grads(agent, D.NAMES)
        got["mult0"] = multiplier_state(agent)

    def on_step(frame):
        got["clip"] = {n: grads_of(net) for n, net in nets.items()}

    def on_after(frame):
        got["mult1"] = multiplier_state(agent)  # after reset_lgr_muls

    tap.on_line["grad"], tap.on_line["step"], tap.on_line["after"] = on_grad, on_step, on_after
    with tap:
        result = agent.learn()
    for h in hooks:
        h.remove()
    assert len(outs["actor"]) == 2 and len(outs["target_actor"]) == 1 and len(outs["critic"]) == 1 and len(outs["target_critic"]) == 2
    n = lambda t: t.detach().numpy().copy()
    out = {"la": n(outs["actor"][0]), "la_next": n(outs["actor"][1]), "la_old": n(outs["target_actor"][0]), "q": n(outs["critic"][0]),
           "qt": n(outs["target_critic"][0]), "qt_next": n(outs["target_critic"][1])}
    tgt, ls = tap.records["target"][0], tap.records["loss"][0]
    out["qret"] = tgt["Qret"].reshape(-1)
    out["qret0"] = tap.records["scan"][0]["Qret"].reshape(-1) if spec["retrace"] and spec["T"] > 1 else out["qret"].copy()
    out["c"] = tgt["c"].reshape(-1)
    for k in ("action", "reward", "prob_b", "state", "next_state"):
        out["in_" + k] = tgt[k]
    out["At"], out["w"], out["kld"] = ls["At"], ls["q"], ls["KLD_pi"]
    for k in ("actor_loss", "critic_loss", "eta_loss", "alpha_loss"):
        out[k] = ls[k]
    out["d_la"], out["d_q"] = got["d_la"], got["d_q"]
    flat("mult0/", got["mult0"], out)
    flat("mult1/", got["mult1"], out)
    flat("mult_grad/", got["mult_grad"], out)
    for net in nets:
        flat(f"grad_raw/{net}/", {k: keep(v) for k, v in got["raw"][net].items()}, out)
        flat(f"grad_clip/{net}/", {k: keep(v) for k, v in got["clip"][net].items()}, out)
        out[f"grad_raw_norm/{net}"] = refkit.grad_norm(got["raw"][net])
        for k, v in got["raw"][net].items():
            out[f"grad_raw_absmax/{net}/{k}"] = np.abs(v).max()
        flat(f"sd1/{net}/", {k: keep(v) for k, v in sd_to_np(nets[net].state_dict()).items()}, out)
    flat("result/", {k: np.asarray(v) for k, v in result.items()}, out)
    return out


def try_fixture(name, replay_seed):
    import torch
    from core.agent.mpo import MPO

    spec = SPECS[name]
    S, A, B, T, N, recipe, limit = spec["S"], spec["A"], spec["B"], spec["T"], spec["N"], spec["recipe"], spec["thin_limit"]
    keep = refkit.keeper(limit)
    refkit.seed_rngs(INIT_SEED)
    agent = MPO(**agent_kwargs(spec))
    assert agent.n_step == T
    nets = {n: getattr(agent, n) for n in D.NETS}
    with torch.no_grad():
        if recipe:
            for n, net in nets.items():
                rec = D.recipe_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, n, RECIPE_SEED, synth)
                for k, p in net.named_parameters():
                    p.copy_(torch.from_numpy(rec[k]))
        else:  # perturb so that pi is not ~uniform (the policy gain is 0.01); the targets sit a little away from their online nets
            for n in ("actor", "critic"):
                for p, pt in zip(nets[n].parameters(), nets["target_" + n].parameters()):
                    p.add_(PERTURB * torch.randn_like(p))
                    pt.copy_(p + PERTURB_TARGET * torch.randn_like(p))
    agent.memory.first_store = False
    done_rows = tuple(range(0, N, 2)) if T > 1 else ()
    rows = D.replay(replay_seed, N, T, S, A, done_rows)
    agent.memory.store(rows)
    out = {}
    for n, net in nets.items():
        sd0 = sd_to_np(net.state_dict())
        if not recipe:
            flat(f"sd0/{n}/", sd0, out)
        for k, v in sd0.items():
            out[f"shape/{n}/{k}"] = np.asarray(v.shape)
    refkit.seed_rngs(NP_SEED)
    ok = True
    for k in range(spec["learns"]):
        state = np.random.get_state()
        idx = np.random.randint(agent.memory.size, size=B)  # replay_buffer.py:26: the draw learn() is about to make
        np.random.set_state(state)
        rec = record_learn(agent, spec, keep)
        rec["idx"] = idx
        cat = lambda key: np.concatenate([rows[i][key] for i in idx], 0).reshape(B * T, -1)
        for key in ("action", "reward", "state", "next_state"):
            assert np.array_equal(rec.pop("in_" + key).reshape(B * T, -1), cat(key).astype(np.float32)), "learn() sampled other rows than the draw predicted"
        assert np.array_equal(rec.pop("in_prob_b").reshape(-1), cat("prob").reshape(-1))
        done = cat("done").reshape(B, T)
        if spec["retrace"]:
            inside = done[:, : T - 1].any(1)
            ok = ok and inside.sum() >= 2 and done[:, T - 2].any()
        ok = ok and (rec["c"] == 1.0).any() and (rec["c"] < 1.0).any()
        flat(f"l{k}/", rec, out)
        print(name, f"l{k}", {key: float(v) for key, v in rec.items() if key.startswith("result/")})
    agent.update_target()
    if name == "mpo_td":
        ok = ok and float(out["l0/mult1/eta"]) == np.float32(spec["floors"][0]) and float(out["l0/mult_grad/eta"]) > 0
    if not recipe:
        for key in D.COLUMNS:
            out[f"in/{key}"] = np.concatenate([r[key] for r in rows], 0)
    hyper = dict(S=S, A=A, H=spec["H"], B=B, T=T, N=N, retrace=int(spec["retrace"]), lr=spec["lr"], gamma=GAMMA, clip_grad_norm=CLIP, learns=spec["learns"], recipe=int(recipe),
                 recipe_seed=RECIPE_SEED, thin_limit=limit, init_seed=INIT_SEED, perturb=PERTURB, perturb_target=PERTURB_TARGET, replay_seed=replay_seed, np_seed=NP_SEED,
                 done_rows=np.asarray(done_rows, np.int64))
    for j, k in enumerate(D.NAMES):
        hyper[k], hyper["min_" + k], hyper["eps_" + k] = spec["mult"][j], spec["floors"][j], spec["eps"][j]
    refkit.put_hyper(out, hyper)
    return out, ok


def gen_fixture(name, out_dir):
    for seed in range(5, 64):
        out, ok = try_fixture(name, seed)
        if ok:
            break
        print(name, f"replay seed {seed}: the sampled batch misses a condition, next seed")
    else:
        raise SystemExit(f"{name}: no replay seed meets the conditions")
    refkit.save_fixture(out_dir, name, out, note=f"replay seed {seed}")


def reference_curve(seed):
    """The reference's single-mode loop (run_mode.py: act, step, interact_callback, process) with its MPO on the oracle's CartPole.
    -> mean reward per step in bins of BIN steps."""
    from core.agent.mpo import MPO

    from oracle.dqn_port import make_env

    c = D.CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = MPO(run_step=c["run_step"], device="cpu", **c["agent"])
    agent.memory.first_store = False
    env, state = make_env(1000 + seed)
    out, acc = [], 0.0
    for step in range(1, c["steps"] + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"]).reshape(-1))
        tr = {"state": state, "next_state": nxt.astype(np.float32), "reward": rew.reshape(1, 1).astype(np.float64), "done": done.reshape(1, 1)}
        tr.update(a)
        tr = agent.interact_callback(tr)
        if tr:
            agent.process([tr], step)
        state = env.obs().astype(np.float32)
        acc += float(rew.reshape(-1)[0])
        if step % BIN == 0:
            out.append(acc / BIN)
            acc = 0.0
    return out


def gen_curves(out_dir, threads):
    seeds = D.CURVE_CONFIG["seeds"]
    doc = refkit.curve_doc("tools/gen_golden_mpo.py --only curves (the unmodified reference MPO, CPU, scratch copy)", seeds, threads,
                           config=D.CURVE_CONFIG, bin=BIN, metric=f"mean reward per step in bins of {BIN} steps (single mode)")
    curves = refkit.seeded_curves(reference_curve, seeds, "mpo", digits=3)
    print("first / last tenth:", [D.curve_tenths(c) for c in curves])
    doc["mpo_cartpole"] = {"reference": curves}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_mpo.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
