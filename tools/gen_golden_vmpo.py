#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of V-MPO, from the UNMODIFIED reference agent (core/agent/vmpo.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs, the hooks, the storage helpers and the on-policy curve loop are
oracle/refkit.py's; this file holds none of the reference's code.

  tests/golden/vmpo_discrete.npz     S 4, A 2, H 32, n_step 8, 5 workers (M 40), B 16: minibatches of 16, 16 and 8 rows.  Multipliers 2.0 / 0.1 / 5.0,
                                     lr 3e-3 (one multiplier step is visible), perturbed weights, every tensor in full; TWO CONSECUTIVE learns l0, l1
  tests/golden/vmpo_continuous.npz   S 5, A 3, H 32, same M and B, one learn; min_alpha_mu = 0.999 under alpha_mu = 1: the first step (gradient
                                     eps_alpha_mu - mean KL = 0.1 > 0, a step of lr down) crosses the floor and is clamped
  tests/golden/vmpo_cartpole.npz     config.vmpo.cartpole exactly (H 512, 8 x 128 = 1024 rows, B 64, lr 2.5e-4, 2.0 / 0.1 / 5.0): recipe weights and a
                                     recipe rollout (regenerated from seeds by the reader), big arrays thinned, one learn
  tests/golden/curves_reference_vmpo.json   CartPole (the oracle's), config.vmpo.cartpole, 8 x 128 x 40 iterations, seeds 1-3: mean episode
                                     length per iteration

A learn `l<k>/` holds the rollout (`in_*`, or its seed and checksums), the pre-pass (`pre/`: old raw heads, value, next_value, adv after the
standardisation), per minibatch `mb<i>/`: idx, the advantages, their lower median and the top-half mask, the four losses, the raw heads and their
gradients, the multipliers with their gradients and Adam moments before and after the step, parameter gradients raw and clipped (first and last
minibatch), and `sd1/` the end weights.  hyper/thin_limit > 0: arrays larger than that are synth.thin(v, limit) samples.
Median condition: the rollout seed is the first (from 5 up) for which, in EVERY recorded minibatch, the next larger advantage lies at least
1e-4 * max |adv| above the lower median -- last-bit differences of another GAE evaluation cannot move a row across the cut.  `hyper/median_gap`
records the smallest relative gap met.

Usage:  python tools/gen_golden_vmpo.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import RECIPE_SEED, LineTap, flat, grads_of, sd_to_np  # noqa: E402

NAMES = ("eta", "alpha_mu", "alpha_sigma")
SPECS = {
    "vmpo_discrete": dict(S=4, A=2, H=32, W=5, T=8, B=16, cont=False, lr=3e-3, lam=0.9, mult=(2.0, 0.1, 5.0), floors=(1e-8, 1e-8, 1e-8), eps=(0.02, 0.1, 0.1),
                          learns=2, recipe=False, thin_limit=0),
    "vmpo_continuous": dict(S=5, A=3, H=32, W=5, T=8, B=16, cont=True, lr=3e-3, lam=0.9, mult=(1.0, 1.0, 1.0), floors=(1e-8, 0.999, 1e-8), eps=(0.01, 0.1, 5e-5),
                            learns=1, recipe=False, thin_limit=0),
    "vmpo_cartpole": dict(S=4, A=2, H=512, W=8, T=128, B=64, cont=False, lr=2.5e-4, lam=0.95, mult=(2.0, 0.1, 5.0), floors=(1e-8, 1e-8, 1e-8), eps=(0.02, 0.1, 0.1),
                          learns=1, recipe=True, thin_limit=8192),
}
GAMMA, CLIP, INIT_SEED, NP_SEED, PERTURB, MEDIAN_GAP = 0.99, 1.0, 11, 21, 0.05, 1e-4
CURVE_CONFIG = dict(workers=8, n_step=128, iterations=40, seeds=(1, 2, 3), run_step=100000,
                    agent=dict(state_size=4, action_size=2, hidden_size=512, network="discrete_policy_value", optim_config={"name": "adam", "lr": 2.5e-4},
                               gamma=0.99, batch_size=64, n_step=128, n_epoch=1, _lambda=0.95, min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.02,
                               eps_alpha_mu=0.1, eps_alpha_sigma=0.1, eta=2.0, alpha_mu=0.1, alpha_sigma=5.0, lr_decay=True))  # config/vmpo/cartpole.py


def agent_kwargs(spec):
    kw = dict(state_size=spec["S"], action_size=spec["A"], hidden_size=spec["H"], network="continuous_policy_value" if spec["cont"] else "discrete_policy_value",
              optim_config={"name": "adam", "lr": spec["lr"]}, gamma=GAMMA, batch_size=spec["B"], n_step=spec["T"], n_epoch=1, _lambda=spec["lam"], clip_grad_norm=CLIP,
              run_step=100000, num_workers=spec["W"], lr_decay=False, device="cpu")
    for j, k in enumerate(NAMES):
        kw[k], kw["min_" + k], kw["eps_" + k] = spec["mult"][j], spec["floors"][j], spec["eps"][j]
    return kw


def multiplier_state(agent):
    return refkit.multiplier_state(agent, NAMES, agent.optimizer)


def record_learn(agent, spec, trs, np_seed, keep):
    """One process() = one learn() of the reference agent (IN PLACE) under the line tap -> (flat dict, smallest relative median gap)."""
    net = agent.network
    tags = {"mu_raw": net.mu, "log_std_raw": net.log_std, "v": net.v} if spec["cont"] else {"logits": net.pi, "v": net.v}
    head_out, hooks = refkit.retaining_hooks(tags)
    markers = {
        "pre": ("ret = adv + value", ["value", "next_value", "adv", "reward", "done"]),
        "mb_loss": ("self.optimizer.zero_grad", ["idx", "_adv", "idx_tophalf", "psi", "actor_loss", "critic_loss", "eta_loss", "alpha_loss", "log_prob"]),
        "mb_grad": ("torch.nn.utils.clip_grad_norm_", []),
        "mb_step": ("self.optimizer.step()", []),
        "mb_after": ("actor_losses.append", []),
    }
    tap = LineTap(type(agent).learn, markers)
    before, after, grads_raw, grads_clip, head_grads, mult_grads = {}, {}, {}, {}, {}, {}
    mbi = lambda: len(tap.records.get("mb_loss", [])) - 1  # keyed by minibatch: a multi-line statement fires its first line more than once

    def on_loss(frame):
        before[mbi() + 1] = multiplier_state(agent)  # (the tap appends this minibatch's record after the callback)

    def on_grad(frame):
        i = mbi()
        grads_raw[i], head_grads[i], mult_grads[i] = grads_of(net), refkit.last_outputs(head_out), refkit.multiplier_grads(agent, NAMES)

    def on_step(frame):
        grads_clip[mbi()] = grads_of(net)

    def on_after(frame):
        after[mbi()] = multiplier_state(agent)

    tap.on_line["mb_loss"], tap.on_line["mb_grad"], tap.on_line["mb_step"], tap.on_line["mb_after"] = on_loss, on_grad, on_step, on_after
    refkit.seed_rngs(np_seed)
    with tap:
        result = agent.process(trs, agent.time_t + spec["T"])
    for h in hooks:
        h.remove()
    assert result, "learn did not run"
    out = {}
    pre = dict(tap.records["pre"][0])
    for tag in tags:
        if tag != "v":
            pre[tag] = head_out[tag][0].detach().numpy().copy()  # the first forward of learn(): the old policy on `state`
    flat("pre/", pre, out)
    nmb = len(tap.records["mb_loss"])
    out["n_minibatch"] = np.asarray(nmb)
    worst_gap = np.inf
    for i in range(nmb):
        rec = dict(tap.records["mb_loss"][i])
        a = rec["_adv"].reshape(-1)
        med = np.sort(a)[(a.size - 1) // 2]
        assert np.array_equal(rec["idx_tophalf"].reshape(-1), a > med), "the lower median is not sorted element (b - 1) // 2"
        above = a[a > med]
        gap = float(above.min() - med) / float(np.abs(a).max()) if above.size else np.inf
        worst_gap = min(worst_gap, gap)
        rec["median"], rec["median_gap"] = np.asarray(med), np.asarray(gap)
        flat(f"mb{i}/", rec, out)
        flat(f"mb{i}/head/", head_grads[i], out)
        flat(f"mb{i}/mult0/", before[i], out)
        flat(f"mb{i}/mult1/", after[i], out)
        flat(f"mb{i}/mult_grad/", mult_grads[i], out)
        if i in (0, nmb - 1):
            flat(f"mb{i}/grad_raw/", {k: keep(v) for k, v in grads_raw[i].items()}, out)
            flat(f"mb{i}/grad_clip/", {k: keep(v) for k, v in grads_clip[i].items()}, out)
            out[f"mb{i}/grad_raw_norm"] = refkit.grad_norm(grads_raw[i])
            for k, v in grads_raw[i].items():
                out[f"mb{i}/grad_raw_absmax/{k}"] = np.abs(v).max()
    flat("result/", {k: np.asarray(v) for k, v in result.items()}, out)
    flat("sd1/", {k: keep(v) for k, v in sd_to_np(net.state_dict()).items()}, out)
    out["np_seed"] = np.asarray(np_seed)
    return out, worst_gap


def try_fixture(name, rollout_seed):
    from core.agent.vmpo import VMPO

    spec = SPECS[name]
    S, A, M, cont, recipe, limit = spec["S"], spec["A"], spec["W"] * spec["T"], spec["cont"], spec["recipe"], spec["thin_limit"]
    keep = refkit.keeper(limit)
    refkit.seed_rngs(INIT_SEED)
    agent = VMPO(**agent_kwargs(spec))
    # without a recipe: perturb the heads so that pi is not ~uniform and the value not ~0 (the policy gain is 0.01)
    refkit.set_weights([agent.network], synth.ppo_recipe if recipe else None, RECIPE_SEED, PERTURB)
    agent.memory.first_store = False
    out = {}
    sd0 = sd_to_np(agent.network.state_dict())
    flat("sd0/", {k: keep(v) for k, v in sd0.items()}, out)
    for k, v in sd0.items():
        out[f"shape/{k}"] = np.asarray(v.shape)
    worst = np.inf
    for k in range(spec["learns"]):
        seed_k = rollout_seed + 100 * k
        trs = synth.ppo_rollout(np.random.RandomState(seed_k), M, S, A, cont, clamp_every=0 if recipe else 17)
        rec, gap = record_learn(agent, spec, trs, NP_SEED + k, keep)
        worst = min(worst, gap)
        flat(f"l{k}/", rec, out)
        out[f"l{k}/rollout_seed"] = np.asarray(seed_k)
        refkit.dump_rollout(out, f"l{k}/", trs, recipe)
        print(name, f"l{k}", {key: float(v) for key, v in rec.items() if key.startswith("result/")}, f"median gap {gap:.3e}")
    hyper = dict(S=S, A=A, H=spec["H"], W=spec["W"], T=spec["T"], B=spec["B"], continuous=int(cont), lr=spec["lr"], gamma=GAMMA, clip_grad_norm=CLIP, learns=spec["learns"],
                 recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit, init_seed=INIT_SEED, perturb=PERTURB, median_gap=worst, clamp_every=0 if recipe else 17)
    hyper["lambda"] = spec["lam"]
    for j, k in enumerate(NAMES):
        hyper[k], hyper["min_" + k], hyper["eps_" + k] = spec["mult"][j], spec["floors"][j], spec["eps"][j]
    refkit.put_hyper(out, hyper)
    return out, worst


def gen_fixture(name, out_dir):
    for seed in range(5, 64):
        out, worst = try_fixture(name, seed)
        if worst >= MEDIAN_GAP:
            break
        print(name, f"rollout seed {seed}: median gap {worst:.3e} < {MEDIAN_GAP}, next seed")
    else:
        raise SystemExit(f"{name}: no rollout seed meets the median condition")
    refkit.save_fixture(out_dir, name, out, note=f"rollout seed {seed}")


def reference_curve(seed):
    """-> (curve, whether alpha_mu reached its floor after some iteration)"""
    from core.agent.vmpo import VMPO

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = VMPO(run_step=c["run_step"], num_workers=c["workers"], device="cpu", **c["agent"])
    floor = []
    curve = refkit.sync_cartpole_curve(agent, seed, c["workers"], c["n_step"], c["iterations"], per_iter=lambda a: floor.append(float(a.alpha_mu.detach()) <= 1e-8))
    return curve, any(floor)


def gen_curves(out_dir, threads):
    doc = refkit.curve_doc("tools/gen_golden_vmpo.py --only curves (the unmodified reference V-MPO, CPU, scratch copy)", CURVE_CONFIG["seeds"], threads,
                           config=CURVE_CONFIG, metric="mean episode length per iteration (transitions / episode ends, 8 x 128 per iteration)")
    floors = []

    def curve(seed):
        c, hit = reference_curve(seed)
        floors.append(bool(hit))
        print("alpha_mu reached its floor:", hit)
        return c

    curves = refkit.seeded_curves(curve, CURVE_CONFIG["seeds"], "vmpo")
    doc["vmpo_cartpole"] = {"reference": curves, "alpha_mu_reached_floor": floors}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_vmpo.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
