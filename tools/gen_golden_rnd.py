#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of RND-PPO, from the UNMODIFIED reference agent (core/agent/rnd_ppo.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs, the storage helpers and the on-policy curve loop are
oracle/refkit.py's; this file holds none of the reference's code.

  tests/golden/rnd_discrete.npz     S 4, A 3, H 32, 2 workers x 8 steps (M 16), B 6: minibatches of 6, 6 and 4 (rnd_truth.SPECS says why not two rows).  All three switches on,
                                    non_episodic off, standardization off, lr 3e-3, perturbed weights, the starting weights in full
  tests/golden/rnd_continuous.npz   S 5, A 2, H 32, same M and B; non_episodic on, standardization on; every fifth action saturated and the
                                    first mu bias moved past the clamp
  tests/golden/rnd_plain.npz        the discrete shapes with obs_normalize, ri_normalize and batch_norm off and non_extrinsic on
  tests/golden/rnd_cartpole.npz     config.rnd_ppo.cartpole exactly (H 512, 8 x 128 rows, B 64, 3 epochs, lr 1e-4): recipe weights and recipe
                                    rollouts (regenerated from seeds by the reader), big arrays thinned
  tests/golden/curves_reference_rnd_ppo.json   CartPole (the oracle's), config.rnd_ppo.cartpole, 8 x 128 x 40 iterations, seeds 1-3: mean
                                    episode length per iteration

Every fixture holds TWO CONSECUTIVE learns l0, l1 (the carry-over of rms_obs, rms_ri, rewems, the four batch norms' running statistics and
both Adam steps).  A learn `l<k>/` holds the rollout (`in_*`, or its seed and checksums), the pre-pass (`pre/`: r_i, value, v_i, the mixed
adv, ret, ret_i, log_prob_old), per minibatch `mb<i>/` idx and the five losses, for the first and the last minibatch the gradients of both
networks as the optimizers saw them (clipped), the result dict, and the end state_dicts of both networks (`sd1/`, `rnd1/`) and the moments of
both optimizers (`opt1/`, `rnd_opt1/`).

The generator checks itself and fails otherwise: the stack handed to rms_ri has T equal rows (the filter hands out its own storage).

Usage:  python tools/gen_golden_rnd.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import RECIPE_SEED, LineTap, flat, grads_of, sd_to_np  # noqa: E402

import rnd_truth as D  # noqa: E402

SPECS = D.SPECS
GAMMA, LAMBDA, CLIP, EPS_CLIP, INIT_SEED, NP_SEED, PERTURB = D.GAMMA, D.LAMBDA, D.CLIP, D.EPS_CLIP, 11, 21, 0.05
CURVE_CONFIG = D.CURVE_CONFIG


def record_learn(agent, spec, trs, np_seed, keep):
    """One process() = one learn() of the reference agent (IN PLACE), observed through the line tap and one wrapped bound method."""
    rnd, T, W = agent.rnd, spec["T"], spec["W"]
    stacks = []
    rms_ri_update = rnd.update_rms_ri

    def rms_ri_tap(v):
        stacks.append(v.detach().numpy().copy())
        return rms_ri_update(v)

    rnd.update_rms_ri = rms_ri_tap
    markers = {
        "pre": ("mean_ret = ret.mean().item()", ["r_i", "value", "v_i", "adv", "ret", "ret_i", "log_prob_old"]),
        "mb": ("self.optimizer.zero_grad(set_to_none=True)", ["idx", "actor_loss", "critic_e_loss", "critic_i_loss", "entropy_loss", "rnd_loss"]),
        "pstep": ("self.optimizer.step()", []),
        "step": ("self.rnd_optimizer.step()", []),
    }
    tap = LineTap(type(agent).learn, markers)
    pgrad, rgrad = {}, {}
    mbi = lambda: len(tap.records.get("mb", [])) - 1
    tap.on_line["pstep"] = lambda frame: pgrad.__setitem__(mbi(), grads_of(agent.network))
    tap.on_line["step"] = lambda frame: rgrad.__setitem__(mbi(), grads_of(rnd, trainable_only=True))
    refkit.seed_rngs(np_seed)
    with tap:
        result = agent.process(trs, agent.time_t + T)
    del rnd.update_rms_ri
    assert result, "learn did not run"
    assert len(stacks) == 1
    stack = stacks[0].reshape(T, W)
    assert all(np.array_equal(stack[0], stack[t]) for t in range(T)), "the recorded stack does not have T equal rows: the reference's filter no longer aliases"
    out = {"stack": stack}
    flat("pre/", {k: np.asarray(v).reshape(-1) for k, v in tap.records["pre"][0].items()}, out)
    nmb = len(tap.records["mb"])
    out["n_minibatch"] = np.asarray(nmb)
    for i in range(nmb):
        flat(f"mb{i}/", dict(tap.records["mb"][i]), out)
        if i in (0, nmb - 1):
            flat(f"mb{i}/grad/", {k: keep(v) for k, v in pgrad[i].items()}, out)
            flat(f"mb{i}/rnd_grad/", {k: keep(v) for k, v in rgrad[i].items()}, out)
    flat("result/", {k: np.asarray(v) for k, v in result.items()}, out)
    flat("sd1/", {k: keep(v) for k, v in sd_to_np(agent.network.state_dict()).items()}, out)
    flat("rnd1/", {k: keep(v) for k, v in sd_to_np(rnd.state_dict()).items()}, out)
    for tag, opt, params in (("opt1", agent.optimizer, list(agent.network.named_parameters())), ("rnd_opt1", agent.rnd_optimizer, list(rnd.named_parameters()))):
        for k, p in params:
            st = opt.state.get(p)
            out[f"{tag}/has_state/{k}"] = np.asarray(int(bool(st)))
            if st:
                out[f"{tag}/exp_avg/{k}"], out[f"{tag}/exp_avg_sq/{k}"] = keep(st["exp_avg"].numpy().copy()), keep(st["exp_avg_sq"].numpy().copy())  # copies: the optimizer goes on writing its tensors
                out[f"{tag}/step"] = np.asarray(int(float(st["step"])))
    out["np_seed"] = np.asarray(np_seed)
    return out


def try_fixture(name):
    import torch
    from core.agent.rnd_ppo import RND_PPO

    spec = SPECS[name]
    S, A, M, cont, recipe, limit = spec["S"], spec["A"], spec["W"] * spec["T"], spec["cont"], spec["recipe"], spec["thin_limit"]
    keep = refkit.keeper(limit)
    refkit.seed_rngs(INIT_SEED)
    agent = RND_PPO(device="cpu", **D.agent_kwargs(spec))
    out = {}
    if not recipe:  # the initial weights one torch.manual_seed(INIT_SEED) gives (the small fixtures: the recipe fixture spends its size on two learns)
        flat("init/", sd_to_np(agent.network.state_dict()), out)
        flat("init_rnd/", sd_to_np(agent.rnd.state_dict()), out)
    refkit.set_weights([agent.network], synth.ppo_recipe if recipe else None, RECIPE_SEED, PERTURB)
    with torch.no_grad():  # then the module's weight tensors, the target's too: its statistics block starts as the reference builds it
        wnames = [k for k, p in agent.rnd.named_parameters() if k.split(".")[0] not in ("rms_obs", "rms_ri", "rff")]
        rec = D.rnd_recipe({k: tuple(p.shape) for k, p in agent.rnd.named_parameters() if k in wnames}, RECIPE_SEED) if recipe else None
        for k, p in agent.rnd.named_parameters():
            if k in wnames:
                p.copy_(torch.from_numpy(rec[k])) if recipe else p.add_(PERTURB * torch.randn_like(p))
        if cont:
            agent.network.mu.bias[0] = 5.5  # a mu past the clamp
    agent.memory.first_store = False
    sd0, rnd0 = sd_to_np(agent.network.state_dict()), sd_to_np(agent.rnd.state_dict())
    keep0 = keep if recipe else (lambda v: v)  # the starting weights in full unless the reader regenerates them from the recipe
    flat("sd0/", {k: keep0(v) for k, v in sd0.items()}, out)
    flat("rnd0/", {k: keep0(v) for k, v in rnd0.items()}, out)
    for k, v in list(sd0.items()) + [("rnd." + k, v) for k, v in rnd0.items()]:
        out[f"shape/{k}"] = np.asarray(v.shape)
    for k in range(spec["learns"]):
        seed_k = 5 + 100 * k
        trs = synth.ppo_rollout(np.random.RandomState(seed_k), M, S, A, cont, clamp_every=5 if cont else 0)
        flat(f"l{k}/", record_learn(agent, spec, trs, NP_SEED + k, keep), out)
        out[f"l{k}/rollout_seed"] = np.asarray(seed_k)
        refkit.dump_rollout(out, f"l{k}/", trs, recipe)
        print(name, f"l{k}", {key[len(f'l{k}/result/'):]: float(v) for key, v in out.items() if key.startswith(f"l{k}/result/")}, flush=True)
    hyper = dict(S=S, A=A, H=spec["H"], W=spec["W"], T=spec["T"], B=spec["B"], continuous=int(cont), lr=spec["lr"], learns=spec["learns"], recipe=int(recipe),
                 recipe_seed=RECIPE_SEED, thin_limit=limit, init_seed=INIT_SEED, perturb=PERTURB, n_epoch=spec["n_epoch"])
    refkit.put_hyper(out, hyper)
    return out


def gen_fixture(name, out_dir):
    refkit.save_fixture(out_dir, name, try_fixture(name), cap=1 << 20)


def reference_curve(seed):
    from core.agent.rnd_ppo import RND_PPO

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = RND_PPO(run_step=c["run_step"], num_workers=c["workers"], device="cpu", **c["agent"])
    return refkit.sync_cartpole_curve(agent, seed, c["workers"], c["n_step"], c["iterations"])


def gen_curves(out_dir, threads):
    doc = refkit.curve_doc("tools/gen_golden_rnd.py --only curves (the unmodified reference RND-PPO, CPU, scratch copy)", CURVE_CONFIG["seeds"], threads,
                           config=CURVE_CONFIG, metric="mean episode length per iteration (transitions / episode ends, 8 x 128 per iteration)")
    doc["rnd_ppo_cartpole"] = {"reference": refkit.seeded_curves(reference_curve, CURVE_CONFIG["seeds"], "rnd_ppo")}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_rnd_ppo.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
