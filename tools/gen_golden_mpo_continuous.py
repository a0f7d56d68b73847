#!/usr/bin/env python3
"""Golden vectors of continuous MPO, from the UNMODIFIED reference agent (core/agent/mpo.py, the continuous branch).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs, the hooks and the storage helpers are oracle/refkit.py's; this
file holds none of the reference's code.

  tests/golden/mpo_cont.npz           S 4, A 3, H 32, B 5 trajectories of T 4 (R 20) out of 12 stored, N 6 samples, Retrace.  Multipliers 2.0 / 0.1 / 0.5,
                                      lr 3e-3, perturbed weights (the targets a little away from their online nets, the mu layer scaled up so that some
                                      raw mu lies beyond +-5), every tensor in full; TWO CONSECUTIVE learns l0, l1, then update_target
  tests/golden/mpo_cont_td.npz        critic_loss_type '1step_TD' (T 1), A 1, N 1: the degenerate E-step (w = 1, At = 0); min_alpha_sigma just under
                                      alpha_sigma and eps_alpha_sigma = 10 (a positive gradient, a step of lr down), so that its first step crosses the floor; one learn
  tests/golden/mpo_cont_pendulum.npz  config.mpo.pendulum exactly (S 3, A 1, H 512, B 64, T 4, N 30, lr 2.5e-4 ... ): recipe weights and a recipe replay,
                                      big arrays thinned, one learn

A learn `l<k>/` holds the sampled rows `idx`, mu / std of online(s), target(s), online(s'), the raw heads of online(s), the sampled z (`zn`, `zt_add`)
with eps = (z - mu) / std evaluated in float64 and rounded to float32, the critic's Q, Qt_a, Qt_next, Qt_add, c, Qret before (`qret0`) and after
(`qret`) the Retrace scan, At, the E-step weights, KLD_mu, KLD_sigma, the four losses, d(loss)/d(raw mu | raw log_std) and d(loss)/dQ, the multipliers
with their gradients and Adam moments before and after the step, both nets' parameter gradients raw and clipped, their end weights `sd1/`, `result/`,
and, as `hyper/ref_<key>_err` (the largest over the fixture's learns), the reference's own float32 error against the float64 truth of tests/mpo_cont_truth.py on its tapped inputs (the GPU tests hold
the kernel to 2 x that + 1e-5 where sums over the samples enter).
Conditions the generator asserts on the SAMPLED batch of mpo_cont (the replay seed is the first from 5 up that meets them): done = 1 inside at least
two trajectories, one of them at position T - 2; c clipped in some rows and unclipped in others; a stored action component exactly +-1; a raw mu of
online(s) beyond +-5.

  tests/golden/curves_reference_mpo_continuous.json   the oracle's control env (S 11, A 3) in single mode, tests/mpo_cont_truth.py's CURVE_CONFIG (H 128,
                                      B 32, T 4, N 8, n_epoch 4), seeds 1-3: mean reward per step in bins of 100 steps

Usage:  python tools/gen_golden_mpo_continuous.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mpo_cont_truth as D  # noqa: E402  (the replay recipe and the float64 truth are shared with the tests)
import mpo_truth as DD  # noqa: E402  (the recipe weights)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import RECIPE_SEED, LineTap, flat, grads_of, sd_to_np  # noqa: E402

SPECS = {
    "mpo_cont": dict(S=4, A=3, H=32, B=5, T=4, N=12, NS=6, retrace=True, lr=3e-3, mult=(2.0, 0.1, 0.5), floors=(1e-8, 1e-8, 1e-8), eps=(0.01, 0.01, 5e-5), learns=2,
                     recipe=False, thin_limit=0, mu_gain=4.0),
    "mpo_cont_td": dict(S=4, A=1, H=32, B=5, T=1, N=12, NS=1, retrace=False, lr=3e-3, mult=(1.0, 0.1, 1.0), floors=(1e-8, 1e-8, 0.999), eps=(0.1, 0.01, 10.0), learns=1,
                        recipe=False, thin_limit=0, mu_gain=4.0),
    "mpo_cont_pendulum": dict(S=3, A=1, H=512, B=64, T=4, N=300, NS=30, retrace=True, lr=2.5e-4, mult=(1.0, 1.0, 1.0), floors=(1e-8, 1e-8, 1e-8), eps=(0.01, 0.01, 5e-5),
                              learns=1, recipe=True, thin_limit=8192, mu_gain=1.0),
}
GAMMA, CLIP, INIT_SEED, NP_SEED, PERTURB, PERTURB_TARGET = 0.99, 1.0, 11, 21, 0.05, 0.02
NETS = ("actor", "target_actor", "critic", "target_critic")


def agent_kwargs(spec):
    kw = dict(state_size=spec["S"], action_size=spec["A"], hidden_size=spec["H"], actor="continuous_policy", critic="continuous_q_network",
              optim_config={"name": "adam", "lr": spec["lr"]}, gamma=GAMMA, buffer_size=max(spec["N"], 64), batch_size=spec["B"], start_train_step=0, n_epoch=spec["learns"],
              n_step=spec["T"] if spec["retrace"] else 8, clip_grad_norm=CLIP, run_step=100000, lr_decay=False, device="cpu", num_sample=spec["NS"],
              critic_loss_type="retrace" if spec["retrace"] else "1step_TD")
    for j, k in enumerate(D.NAMES):
        kw[k], kw["min_" + k], kw["eps_" + k] = spec["mult"][j], spec["floors"][j], spec["eps"][j]
    return kw


def record_learn(agent, spec, keep):
    """One learn() of the reference agent (IN PLACE) under the line tap -> flat dict."""
    outs, hooks = refkit.retaining_hooks({"mu": agent.actor.mu, "log_std": agent.actor.log_std, "critic": agent.critic.q})
    held = ["mu", "std", "mut", "stdt", "next_mu", "next_std", "zn", "zt_add", "Q", "Qt_a", "Qt_next", "Qt_add", "c", "Qret", "action", "reward", "prob_b", "state",
            "next_state", "done"]
    markers = {
        "scan": ("for i in reversed(range(Qret.shape[1] - 1)):", ["Qret"]),  # the continuous branch's loop header: first hit = before the scan
        "target": ("critic_loss = F.mse_loss(Q, Qret)", held),
        "loss": ("loss = critic_loss + actor_loss", ["At", "q", "KLD_mu", "KLD_sigma", "actor_loss", "critic_loss", "eta_loss", "alpha_loss"]),
        "grad": ("torch.nn.utils.clip_grad_norm_(self.actor.parameters()", []),
        "step": ("self.actor_optimizer.step()", []),
        "after": ("self.num_learn += 1", []),
    }
    tap = LineTap(type(agent).learn, markers)
    nets = {"actor": agent.actor, "critic": agent.critic}
    got = {}

    def on_grad(frame):
        got["raw"] = {n: grads_of(net) for n, net in nets.items()}
        got["d_head"] = np.concatenate([outs["mu"][0].grad.detach().numpy(), outs["log_std"][0].grad.detach().numpy()], 1)
        got["head"] = np.concatenate([outs["mu"][0].detach().numpy(), outs["log_std"][0].detach().numpy()], 1)
        got["d_q"] = outs["critic"][0].grad.detach().numpy().reshape(-1).copy()
        got["mult_grad"] = refkit.multiplier_grads(agent, D.NAMES)
        got["mult0"] = refkit.multiplier_state(agent, D.NAMES, agent.actor_optimizer)

    def on_step(frame):
        got["clip"] = {n: grads_of(net) for n, net in nets.items()}

    def on_after(frame):
        got["mult1"] = refkit.multiplier_state(agent, D.NAMES, agent.actor_optimizer)  # after reset_lgr_muls

    tap.on_line["grad"], tap.on_line["step"], tap.on_line["after"] = on_grad, on_step, on_after
    with tap:
        result = agent.learn()
    for h in hooks:
        h.remove()
    assert len(outs["mu"]) == 2 and len(outs["critic"]) == 1
    tgt, ls = tap.records["target"][0], tap.records["loss"][0]
    R, A, NS = spec["B"] * spec["T"], spec["A"], spec["NS"]
    out = {"head": got["head"], "d_head": got["d_head"], "d_q": got["d_q"]}
    for k in ("mu", "std", "mut", "stdt", "next_mu", "next_std"):
        out[k] = np.asarray(tgt[k]).reshape(R, A)
    out["zn"], out["zt_add"] = np.asarray(tgt["zn"]).reshape(NS, R, A), np.asarray(tgt["zt_add"]).reshape(NS, R, A)
    f64 = lambda k: np.asarray(tgt[k]).astype(np.float64)
    out["eps"] = np.stack([(f64("zn").reshape(NS, R, A) - f64("next_mu").reshape(R, A)) / f64("next_std").reshape(R, A),
                           (f64("zt_add").reshape(NS, R, A) - f64("mut").reshape(R, A)) / f64("stdt").reshape(R, A)]).astype(np.float32)
    out["q"], out["qt_a"] = np.asarray(tgt["Q"]).reshape(R), np.asarray(tgt["Qt_a"]).reshape(R)
    out["qt_next"], out["qt_add"] = np.asarray(tgt["Qt_next"]).reshape(NS, R), np.asarray(tgt["Qt_add"]).reshape(NS, R)
    out["qret"] = np.asarray(tgt["Qret"]).reshape(-1)
    out["qret0"] = np.asarray(tap.records["scan"][0]["Qret"]).reshape(-1) if spec["retrace"] and spec["T"] > 1 else out["qret"].copy()
    out["c"] = np.asarray(tgt["c"]).reshape(-1)
    for k in ("action", "reward", "prob_b", "state", "next_state", "done"):
        out["in_" + k] = np.asarray(tgt[k])
    out["At"], out["w"] = np.asarray(ls["At"]).reshape(NS, R), np.asarray(ls["q"]).reshape(NS, R)
    out["kld_mu"], out["kld_sigma"] = np.asarray(ls["KLD_mu"]).reshape(R), np.asarray(ls["KLD_sigma"]).reshape(R)
    for k in ("actor_loss", "critic_loss", "eta_loss", "alpha_loss"):
        out[k] = ls[k]
    flat("mult0/", got["mult0"], out)
    flat("mult1/", got["mult1"], out)
    flat("mult_grad/", got["mult_grad"], out)
    for net in nets:
        flat(f"grad_raw/{net}/", got["raw"][net], out)
        flat(f"grad_clip/{net}/", got["clip"][net], out)
        out[f"grad_raw_norm/{net}"] = refkit.grad_norm(got["raw"][net])
        for k, v in got["raw"][net].items():
            out[f"grad_raw_absmax/{net}/{k}"] = np.abs(v).max()
        flat(f"sd1/{net}/", sd_to_np(nets[net].state_dict()), out)
    flat("result/", {k: np.asarray(v) for k, v in result.items()}, out)
    # the reference's own float32 error against the float64 truth on ITS tapped inputs
    mult0 = [float(got["mult0"][n]) for n in D.NAMES]
    t = D.loss(out["head"], np.concatenate([np.asarray(tgt["mut"]).reshape(R, A), np.arctanh(np.log(np.asarray(tgt["stdt"]).astype(np.float64))).reshape(R, A)], 1),
               out["q"], out["qt_a"], out["qt_next"], out["qt_add"], out["zt_add"], out["in_action"], out["in_reward"], out["in_done"], out["in_prob_b"], spec["T"], mult0,
               spec["eps"], GAMMA, spec["retrace"])
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64).reshape(np.shape(b)) - b).max() / (np.abs(b).max() + 1e-30))
    err = {"actor_loss": rel(out["actor_loss"], t["actor"]), "critic_loss": rel(out["critic_loss"], t["critic"]), "eta_loss": rel(out["eta_loss"], t["eta_loss"]),
           "alpha_loss": rel(out["alpha_loss"], t["alpha_loss"]), "qret": rel(out["qret"], t["qret"]), "At": rel(out["At"], t["At"]), "w": rel(out["w"], t["w"]),
           "d_head": rel(out["d_head"], t["grads"]["head"]), "d_q": rel(out["d_q"], t["grads"]["q"])}
    # thinned ONCE, here (hyper/thin_limit; the inputs and the normals stay whole)
    out = {k: (keep(v) if isinstance(v, np.ndarray) and v.ndim > 0 and not k.startswith(("in_", "idx", "eps")) else v) for k, v in out.items()}  # eps stays whole: the tests inject it
    return out, t, err


def try_fixture(name, replay_seed):
    import torch
    from core.agent.mpo import MPO

    spec = SPECS[name]
    S, A, B, T, N, recipe, limit = spec["S"], spec["A"], spec["B"], spec["T"], spec["N"], spec["recipe"], spec["thin_limit"]
    keep = refkit.keeper(limit)
    refkit.seed_rngs(INIT_SEED)
    agent = MPO(**agent_kwargs(spec))
    assert agent.n_step == T and agent.action_type == "continuous"
    nets = {n: getattr(agent, n) for n in NETS}
    with torch.no_grad():
        if recipe:
            for n, net in nets.items():
                rec = DD.recipe_weights({k: tuple(v.shape) for k, v in net.state_dict().items()}, n, RECIPE_SEED, synth)
                for k, p in net.named_parameters():
                    p.copy_(torch.from_numpy(rec[k]))
        else:  # perturbed; the targets sit a little away from their online nets; the mu layer scaled so that some raw mu passes the +-5 clamp
            for n in ("actor", "critic"):
                for p, pt in zip(nets[n].parameters(), nets["target_" + n].parameters()):
                    p.add_(PERTURB * torch.randn_like(p))
                    pt.copy_(p + PERTURB_TARGET * torch.randn_like(p))
            for net in (nets["actor"], nets["target_actor"]):
                net.mu.weight.mul_(spec["mu_gain"])
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
    ok, ref_err = True, {}
    for k in range(spec["learns"]):
        state = np.random.get_state()
        idx = np.random.randint(agent.memory.size, size=B)  # replay_buffer.py:26: the draw learn() is about to make
        np.random.set_state(state)
        rec, t, err = record_learn(agent, spec, keep)
        ref_err = {key: max(v, ref_err.get(key, 0.0)) for key, v in err.items()}
        rec["idx"] = idx
        cat = lambda key: np.concatenate([rows[i][key] for i in idx], 0).reshape(B * T, -1)
        for key in ("action", "reward", "state", "next_state"):
            assert np.array_equal(rec.pop("in_" + key).reshape(B * T, -1), cat(key).astype(np.float32)), "learn() sampled other rows than the draw predicted"
        assert np.array_equal(rec.pop("in_prob_b").reshape(-1), cat("prob").reshape(-1))
        rec.pop("in_done")
        if name == "mpo_cont":
            done = cat("done").reshape(B, T)
            clip, clamp = D.distance_from_the_switches(t)
            ok = ok and done[:, : T - 1].any(1).sum() >= 2 and done[:, T - 2].any() and (rec["c"] == 1.0).any() and (rec["c"] < 1.0).any()
            ok = ok and (np.abs(cat("action")) == 1.0).any() and (np.abs(rec["head"][:, :A]) > 5.0).any() and clip > 1e-4 and clamp > 1e-4
        flat(f"l{k}/", rec, out)
        print(name, f"l{k}", {key: float(v) for key, v in rec.items() if key.startswith("result/")}, err)
    agent.update_target()
    if name == "mpo_cont_td":
        ok = ok and float(out["l0/mult1/alpha_sigma"]) == np.float32(spec["floors"][2]) and not out["l0/At"].any() and (out["l0/w"] == 1.0).all()
    hyper = dict(S=S, A=A, H=spec["H"], B=B, T=T, N=N, NS=spec["NS"], retrace=int(spec["retrace"]), lr=spec["lr"], gamma=GAMMA, clip_grad_norm=CLIP, learns=spec["learns"],
                 recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit, init_seed=INIT_SEED, perturb=PERTURB, perturb_target=PERTURB_TARGET, mu_gain=spec["mu_gain"],
                 replay_seed=replay_seed, np_seed=NP_SEED, done_rows=np.asarray(done_rows, np.int64))
    for j, k in enumerate(D.NAMES):
        hyper[k], hyper["min_" + k], hyper["eps_" + k] = spec["mult"][j], spec["floors"][j], spec["eps"][j]
    hyper.update({f"ref_{key}_err": v for key, v in ref_err.items()})  # the largest over the learns
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
    refkit.save_fixture(out_dir, name, out, cap=1 << 20, note=f"replay seed {seed}")


def reference_curve(seed):
    """The reference's single-mode loop with its continuous MPO on the oracle's control env -> mean reward per step in bins."""
    from core.agent.mpo import MPO

    from oracle.jorldy_oracle import ControlOracle

    c = D.CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = MPO(run_step=c["run_step"], device="cpu", **c["agent"])
    agent.memory.first_store = False
    return D.control_curve(agent, ControlOracle(1, c["S"], c["A"], seed=1000 + seed), c["steps"], c["bin"])


def gen_curves(out_dir, threads):
    seeds = D.CURVE_CONFIG["seeds"]
    doc = refkit.curve_doc("tools/gen_golden_mpo_continuous.py --only curves (the unmodified reference MPO, continuous branch, CPU, scratch copy)", seeds, threads,
                           config=D.CURVE_CONFIG, metric=f"mean reward per step in bins of {D.CURVE_CONFIG['bin']} steps (single mode, the oracle's control env)")
    curves = refkit.seeded_curves(reference_curve, seeds, "mpo_continuous", digits=3)
    print("first / last tenth:", [D.curve_tenths(c) for c in curves])
    doc["mpo_control"] = {"reference": curves}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_mpo_continuous.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
