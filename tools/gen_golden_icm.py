#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of ICM-PPO, from the UNMODIFIED reference agent (core/agent/icm_ppo.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs, the storage helpers and the on-policy curve loop are
oracle/refkit.py's; this file holds none of the reference's code.

  tests/golden/icm_discrete.npz     S 4, A 2, H 32, 5 workers x 8 steps (M 40), B 16: minibatches of 16, 16 and 8.  All three switches on, lr 3e-3,
                                    perturbed weights, the starting weights in full, recorded arrays over 4096 entries thinned; TWO CONSECUTIVE learns l0, l1 (the carry-over of rms_obs, rms_ri,
                                    rewems, the running statistics and the Adam step)
  tests/golden/icm_continuous.npz   S 5, A 3, H 32, same M and B, one learn
  tests/golden/icm_plain.npz        the discrete shapes with obs_normalize, ri_normalize and batch_norm off
  tests/golden/icm_cartpole.npz     config.icm_ppo.cartpole exactly (H 512, 8 x 128 rows, B 32, 3 epochs, lr 2.5e-4): recipe weights and a recipe
                                    rollout (regenerated from seeds by the reader), big arrays thinned, one learn
  tests/golden/curves_reference_icm_ppo.json   CartPole (the oracle's), config.icm_ppo.cartpole, 8 x 128 x 40 iterations, seeds 1-3: mean
                                    episode length per iteration

A learn `l<k>/` holds the rollout (`in_*`, or its seed and checksums), the statistics block before the learn (`blk0/`; after it: in `icm1/`), raw
r_i, the stacked rewems AS THE REFERENCE BUILT IT, normalised r_i, the mixed reward, PPO's pre-pass (`pre/`), per minibatch `mb<i>/` idx, l_f, l_i
and PPO's three losses, for the first and the last minibatch the inputs of each batch norm and the ICM's gradients raw and clipped, the result
dict, and the end state_dicts of both networks (`sd1/`, `icm1/`) and the moments of both optimizers (`opt1/`, `icm_opt1/`).

The generator checks itself and fails otherwise:
  * the recorded stack has T equal rows (RewardForwardFilter.update returns the Parameter itself);
  * the per-step filter states would have given an rms_ri.var that differs from the recorded one by more than 1e-3 relative: the aliasing is
    visible in the fixture;
  * tests/icm_truth.py in float64, driven over every minibatch of every learn with its own Adam, ends within HALF of the caps the GPU test puts on
    the ICM's end weights (0.25 % of entries further than 2e-5, the worst within 1.05 lr).  INIT_SEED is chosen accordingly.

Usage:  python tools/gen_golden_icm.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import RECIPE_SEED, LineTap, flat, grads_of, sd_to_np  # noqa: E402

SPECS = {
    "icm_discrete": dict(S=4, A=2, H=32, W=5, T=8, B=16, cont=False, lr=3e-3, n_epoch=1, on=True, learns=2, recipe=False, thin_limit=4096, std=True, eta=0.1),
    "icm_continuous": dict(S=5, A=3, H=32, W=5, T=8, B=16, cont=True, lr=3e-3, n_epoch=1, on=True, learns=1, recipe=False, thin_limit=4096, std=True, eta=0.1),
    "icm_plain": dict(S=4, A=2, H=32, W=5, T=8, B=16, cont=False, lr=3e-3, n_epoch=1, on=False, learns=1, recipe=False, thin_limit=4096, std=True, eta=0.1),
    "icm_cartpole": dict(S=4, A=2, H=512, W=8, T=128, B=32, cont=False, lr=2.5e-4, n_epoch=3, on=True, learns=1, recipe=True, thin_limit=8192, std=False, eta=0.1),
}
GAMMA, LAMBDA, CLIP, EPS_CLIP, VF, ENT, BETA, INIT_SEED, NP_SEED, PERTURB = 0.99, 0.95, 1.0, 0.1, 1.0, 0.01, 0.2, 11, 21, 0.05
CURVE_CONFIG = dict(workers=8, n_step=128, iterations=40, seeds=(1, 2, 3), run_step=100000,
                    agent=dict(state_size=4, action_size=2, hidden_size=512, network="discrete_policy_value", head="mlp", optim_config={"name": "adam", "lr": 2.5e-4},
                               gamma=0.99, batch_size=32, n_step=128, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, clip_grad_norm=1.0,
                               use_standardization=False, lr_decay=True, icm_network="icm_mlp", beta=0.2, lamb=1.0, eta=0.1, extrinsic_coeff=1.0,
                               intrinsic_coeff=1.0))  # config/icm_ppo/cartpole.py
BNS = ("bn1", "bn2", "bn1_next")


def agent_kwargs(spec):
    return dict(state_size=spec["S"], action_size=spec["A"], hidden_size=spec["H"], network="continuous_policy_value" if spec["cont"] else "discrete_policy_value",
                head="mlp", optim_config={"name": "adam", "lr": spec["lr"]}, gamma=GAMMA, batch_size=spec["B"], n_step=spec["T"], n_epoch=spec["n_epoch"], _lambda=LAMBDA,
                epsilon_clip=EPS_CLIP, vf_coef=VF, ent_coef=ENT, clip_grad_norm=CLIP, use_standardization=spec["std"], run_step=100000, num_workers=spec["W"],
                lr_decay=False, device="cpu", icm_network="icm_mlp", beta=BETA, lamb=1.0, eta=spec["eta"], extrinsic_coeff=1.0, intrinsic_coeff=1.0,
                obs_normalize=spec["on"], ri_normalize=spec["on"], batch_norm=spec["on"])


def record_learn(agent, spec, trs, np_seed, keep):
    """One process() = one learn() of the reference agent (IN PLACE), observed through the line tap, forward hooks and two wrapped bound methods."""
    import torch

    import icm_truth as D

    icm, W = agent.icm, spec["W"]
    seen = {"rff_in": [], "stack": [], "bn_in": {k: [] for k in BNS}}
    rff_update, rms_ri_update = icm.rff.update, icm.update_rms_ri

    def rff_tap(rews):
        seen["rff_in"].append(rews.detach().numpy().copy())
        return rff_update(rews)

    def rms_ri_tap(v):
        seen["stack"].append(v.detach().numpy().copy())
        return rms_ri_update(v)

    icm.rff.update, icm.update_rms_ri = rff_tap, rms_ri_tap
    hooks = []
    if spec["on"]:
        for k in BNS:
            hooks.append(getattr(icm, k).register_forward_hook(lambda mod, inp, outp, k=k: seen["bn_in"][k].append(inp[0].detach().numpy().copy())))
    markers = {
        "mix": ("self.extrinsic_coeff * reward", ["r_i"]),
        "pre": ("ret = adv.view(-1, 1) + value", ["value", "next_value", "adv", "reward", "log_prob_old"]),
        "mb": ("icm_loss = self.beta * l_f", ["idx", "l_f", "l_i", "actor_loss", "critic_loss", "entropy_loss"]),
        "clip": ("self.icm.parameters(), self.clip_grad_norm", []),
        "step": ("self.icm_optimizer.step()", []),
    }
    tap = LineTap(type(agent).learn, markers)
    raw, clipped = {}, {}
    mbi = lambda: len(tap.records.get("mb", [])) - 1
    tap.on_line["clip"] = lambda frame: raw.__setitem__(mbi(), grads_of(icm, trainable_only=True))
    tap.on_line["step"] = lambda frame: clipped.__setitem__(mbi(), grads_of(icm, trainable_only=True))
    blk0 = sd_to_np(icm.state_dict())
    icm0 = {k: v.copy() for k, v in blk0.items()}
    refkit.seed_rngs(np_seed)
    with tap:
        result = agent.process(trs, agent.time_t + spec["T"])
    for h in hooks:
        h.remove()
    del icm.rff.update, icm.update_rms_ri
    assert result, "learn did not run"
    T = spec["T"]
    out = {}
    flat("blk0/", {k: blk0[k] for k in blk0 if k.split(".")[0] in ("rms_obs", "rms_ri", "rff") or "running" in k or "num_batches" in k}, out)
    r_raw = np.stack(seen["rff_in"]).T.reshape(-1)  # [T][W] arguments of rff.update -> r_i.view(W, -1) order
    stack = seen["stack"][0].reshape(T, W)
    assert len(seen["rff_in"]) == T and len(seen["stack"]) == 1
    assert all(np.array_equal(stack[0], stack[t]) for t in range(T)), "the recorded stack does not have T equal rows: the reference's filter no longer aliases"
    out["r_raw"], out["stack"] = r_raw, stack
    out["r_i"] = tap.records["mix"][0]["r_i"]
    true_stack = D.filter_states(blk0["rff.rewems"], r_raw.reshape(W, T), GAMMA, torch.float32)
    _, v_true, _ = D.moments_merge(blk0["rms_ri.mean"], blk0["rms_ri.var"], blk0["rms_ri.count"], true_stack.reshape(-1, 1), torch.float32)
    pre = dict(tap.records["pre"][0])
    nmb = len(tap.records["mb"])
    # rms_ri is written once per learn (by the pre-pass), so its variance after the whole learn is the one this stack produced
    v_rec = float(np.asarray(sd_to_np(icm.state_dict())["rms_ri.var"]).reshape(-1)[0])
    gap = abs(float(v_true) - v_rec) / abs(v_rec)
    assert gap > 1e-3, f"the aliasing is invisible in this fixture: rms_ri.var {v_rec} vs {float(v_true)} from the per-step states"
    out["alias_gap"] = np.asarray(gap)
    flat("pre/", pre, out)
    out["n_minibatch"] = np.asarray(nmb)
    for i in range(nmb):
        flat(f"mb{i}/", dict(tap.records["mb"][i]), out)
        if i in (0, nmb - 1):
            flat(f"mb{i}/grad_raw/", {k: keep(v) for k, v in raw[i].items()}, out)
            flat(f"mb{i}/grad_clip/", {k: keep(v) for k, v in clipped[i].items()}, out)
            out[f"mb{i}/grad_raw_norm"] = refkit.grad_norm(raw[i])
            if spec["on"]:  # forward 0 of each batch norm is the pre-pass over the whole rollout, forward 1 + i is minibatch i
                flat(f"mb{i}/bn_in/", {k: keep(seen["bn_in"][k][1 + i]) for k in BNS}, out)
    flat("result/", {k: np.asarray(v) for k, v in result.items()}, out)
    flat("sd1/", {k: keep(v) for k, v in sd_to_np(agent.network.state_dict()).items()}, out)
    icm1 = sd_to_np(icm.state_dict())
    flat("icm1/", {k: keep(v) for k, v in icm1.items()}, out)
    for tag, opt, params in (("opt1", agent.optimizer, list(agent.network.named_parameters())), ("icm_opt1", agent.icm_optimizer, list(icm.named_parameters()))):
        for k, p in params:
            st = opt.state.get(p)
            out[f"{tag}/has_state/{k}"] = np.asarray(int(bool(st)))
            if st:
                out[f"{tag}/exp_avg/{k}"], out[f"{tag}/exp_avg_sq/{k}"] = keep(st["exp_avg"].numpy()), keep(st["exp_avg_sq"].numpy())
                out[f"{tag}/step"] = np.asarray(int(float(st["step"])))
    out["np_seed"] = np.asarray(np_seed)
    return out, icm0, icm1, [tap.records["mb"][i]["idx"] for i in range(nmb)]


def truth_end_weights(spec, icm0, trs, idx_lists, dtype):
    """tests/icm_truth.py over one learn: the pre-pass, then every minibatch with its own Adam.  -> (end trainable weights, block after)"""
    import torch

    import icm_truth as D

    cfg = D.config(spec["S"], spec["A"], spec["H"], spec["cont"], W=spec["W"], gamma=GAMMA, eta=spec["eta"], obs_norm=spec["on"], ri_norm=spec["on"], bn=spec["on"])
    cols = {k: np.concatenate([t[k] for t in trs], 0).astype(np.float32) for k in ("state", "action", "next_state", "reward")}
    names = list(D.shapes(cfg))
    P = {k: torch.nn.Parameter(torch.as_tensor(icm0[k]).to(dtype)) for k in names}
    blk = {k: icm0[k] for k in D.BLOCK_KEYS if k in icm0}
    for k in D.BLOCK_KEYS:
        blk.setdefault(k, D.fresh_block(cfg)[k])
    opt = torch.optim.Adam(list(P.values()), lr=spec["lr"])
    if icm0.get("_opt"):
        opt.load_state_dict(icm0["_opt"])
    out = D.reward_pass(cfg, {k: p.detach() for k, p in P.items()}, blk, cols["state"], cols["action"], cols["next_state"], cols["reward"], dtype=dtype)
    blk = {k: np.asarray(v.detach().double()) for k, v in out["block"].items()}
    losses = []
    for idx in idx_lists:
        u = D.update(cfg, {k: p.detach() for k, p in P.items()}, blk, cols["state"][idx], cols["action"][idx], cols["next_state"][idx], BETA, CLIP, dtype)
        for k, p in P.items():
            p.grad = u["clipped"][k].reshape(p.shape).clone()
        opt.step()
        for k, v in u["run"].items():
            blk[k] = np.asarray(v.detach().double())
        losses.append((float(u["l_f"]), float(u["l_i"])))
    out["losses"] = losses
    return {k: p.detach().double().numpy() for k, p in P.items()}, blk, opt, out


def try_fixture(name):
    import torch
    from core.agent.icm_ppo import ICM_PPO

    import icm_truth as D

    spec = SPECS[name]
    S, A, M, cont, recipe, limit = spec["S"], spec["A"], spec["W"] * spec["T"], spec["cont"], spec["recipe"], spec["thin_limit"]
    keep = refkit.keeper(limit)
    refkit.seed_rngs(INIT_SEED)
    agent = ICM_PPO(**agent_kwargs(spec))
    refkit.set_weights([agent.network], synth.ppo_recipe if recipe else None, RECIPE_SEED, PERTURB)
    with torch.no_grad():  # then the ICM's trainable tensors alone: its statistics block starts as the reference builds it
        rec = D.icm_recipe({k: tuple(p.shape) for k, p in agent.icm.named_parameters() if p.requires_grad}, RECIPE_SEED) if recipe else None
        for k, p in agent.icm.named_parameters():
            if p.requires_grad:
                p.copy_(torch.from_numpy(rec[k])) if recipe else p.add_(PERTURB * torch.randn_like(p))
    agent.memory.first_store = False
    out = {}
    sd0, icm0 = sd_to_np(agent.network.state_dict()), sd_to_np(agent.icm.state_dict())
    keep0 = keep if recipe else (lambda v: v)  # the starting weights in full unless the reader regenerates them from the recipe
    flat("sd0/", {k: keep0(v) for k, v in sd0.items()}, out)
    flat("icm0/", {k: keep0(v) for k, v in icm0.items()}, out)
    for k, v in list(sd0.items()) + [("icm." + k, v) for k, v in icm0.items()]:
        out[f"shape/{k}"] = np.asarray(v.shape)
    t_w, t_blk, t_opt = None, None, None
    for k in range(spec["learns"]):
        seed_k = 5 + 100 * k
        trs = synth.ppo_rollout(np.random.RandomState(seed_k), M, S, A, cont, clamp_every=0)
        rec, icm_before, icm_after, idx_lists = record_learn(agent, spec, trs, NP_SEED + k, keep)
        flat(f"l{k}/", rec, out)
        out[f"l{k}/rollout_seed"] = np.asarray(seed_k)
        refkit.dump_rollout(out, f"l{k}/", trs, recipe)
        # the float64 truth over the same learn, continued from its own previous end: within half of the GPU test's caps
        start = dict(icm_before) if t_w is None else {**{kk: np.asarray(v, np.float64) for kk, v in t_blk.items()}, **t_w}
        if t_opt is not None:
            start["_opt"] = t_opt.state_dict()
        t_w, t_blk, t_opt, t_pre = truth_end_weights(spec, start, trs, idx_lists, torch.float64)
        tot = bad = 0
        worst = 0.0
        for kk, v in t_w.items():
            dd = np.abs(v - icm_after[kk].astype(np.float64))
            tot, bad, worst = tot + dd.size, bad + int((dd > 2e-5).sum()), max(worst, float(dd.max()) / spec["lr"])
        e_ri = D.rel(rec["r_i"], t_pre["r_i"])
        # how far the reference's own float32 losses drift from the float64 chain over the minibatches: four times this is the GPU test's bound on them
        dev = max(abs(float(rec[f"mb{i}/{key}"]) - t) / abs(t) for i, pair in enumerate(t_pre["losses"]) for key, t in zip(("l_f", "l_i"), pair))
        out[f"l{k}/truth_loss_dev"] = np.asarray(dev)
        print(name, f"l{k}", {key[7:]: float(v) for key, v in rec.items() if key.startswith("result/")}, f"alias gap {float(rec['alias_gap']):.3e}",
              f"| truth vs reference: r_i {e_ri:.2e}, losses {dev:.2e}, end weights {bad}/{tot} beyond 2e-5, worst {worst:.3f} lr", flush=True)
        assert e_ri <= 0.5e-5 and bad / tot <= 0.0025 and worst <= 1.05, "the float64 truth does not stay within half of the GPU test's caps: pick another INIT_SEED"
        out[f"l{k}/truth_bad_fraction"], out[f"l{k}/truth_worst_lr"] = np.asarray(bad / tot), np.asarray(worst)
    hyper = dict(S=S, A=A, H=spec["H"], W=spec["W"], T=spec["T"], B=spec["B"], continuous=int(cont), lr=spec["lr"], gamma=GAMMA, clip_grad_norm=CLIP, learns=spec["learns"],
                 recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit, init_seed=INIT_SEED, perturb=PERTURB, n_epoch=spec["n_epoch"], epsilon_clip=EPS_CLIP,
                 vf_coef=VF, ent_coef=ENT, beta=BETA, eta=spec["eta"], switches=int(spec["on"]), use_standardization=int(spec["std"]))
    hyper["lambda"] = LAMBDA
    refkit.put_hyper(out, hyper)
    return out


def gen_fixture(name, out_dir):
    refkit.save_fixture(out_dir, name, try_fixture(name))


def reference_curve(seed):
    from core.agent.icm_ppo import ICM_PPO

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = ICM_PPO(run_step=c["run_step"], num_workers=c["workers"], device="cpu", **c["agent"])
    return refkit.sync_cartpole_curve(agent, seed, c["workers"], c["n_step"], c["iterations"])


def gen_curves(out_dir, threads):
    doc = refkit.curve_doc("tools/gen_golden_icm.py --only curves (the unmodified reference ICM-PPO, CPU, scratch copy)", CURVE_CONFIG["seeds"], threads,
                           config=CURVE_CONFIG, metric="mean episode length per iteration (transitions / episode ends, 8 x 128 per iteration)")
    doc["icm_ppo_cartpole"] = {"reference": refkit.seeded_curves(reference_curve, CURVE_CONFIG["seeds"], "icm_ppo")}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_icm_ppo.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
