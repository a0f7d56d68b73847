#!/usr/bin/env python3
"""Golden vectors and the reference learning curve of R2D2, from the UNMODIFIED reference agent (core/agent/r2d2.py, core/network/r2d2.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or reads
the reference.  Staging, the main, the line tap under which `R2D2.learn()` runs and the storage helpers are oracle/refkit.py's; this file
holds none of the reference's code.

Every fixture: the reference agent with recipe weights (synth.recipe_state_dict, seed and seed + 1 for online and target; l2_a / l2_v scaled by
hyper/q_scale so that |target Q| is 5 or more where asked), its buffer filled by ITS OWN act / interact_callback loop on synthetic states with
an episode end every hyper/episode steps (states, rewards from RandomState(fill_seed); the epsilon draws from np.random seeded with
hyper/act_np_seed), then two consecutive learn()s under np / torch seed 42.  Recorded: init_thin/ (a fresh agent's initial weights under
torch seed 5), the acting trace of the first hyper/trace steps (across an episode end), every stored row (rows/, thinned where large) with its actor priority and
the tree after the fill, and per learn l<k>/: the tapped q, q_pred, next_q, next_target_q, target_q, td_error, priority, p_j, indices,
weights, loss, the result, gradients, weights, Adam moments (thinned) and the sum tree after the write-back.  hyper/ref_target_err: the
distance of the reference's float32 target_q from the float64 evaluation of the same expression on the same inputs, relative to the largest
entry.

  tests/golden/r2d2.npz            S 4, A 3, H 64, B 8, seq 4, burn 1, n_step 3, padding on
  tests/golden/r2d2_odd.npz        S 5, A 5, H 36, B 7, seq 6, burn 3, n_step 2, padding off
  tests/golden/r2d2_cartpole.npz   config.r2d2.cartpole exactly (H 512, B 64, Adam 1e-4, clip 40)
  tests/golden/curves_reference_r2d2.json   config.r2d2.cartpole in run_mode's single loop on the oracle's CartPole, three seeds

Usage:  python tools/gen_golden_r2d2.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 8]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED  # noqa: E402

SPECS = {
    "r2d2": dict(S=4, A=3, H=64, B=8, seq=4, burn=1, n=3, pad=True, lr=1e-3, beta=0.4, steps=60, episode=11, q_scale=24.0, stride=61),
    "r2d2_odd": dict(S=5, A=5, H=36, B=7, seq=6, burn=3, n=2, pad=False, lr=1e-3, beta=0.4, steps=160, episode=7, q_scale=32.0, stride=61),
    "r2d2_cartpole": dict(S=4, A=2, H=512, B=64, seq=4, burn=1, n=3, pad=True, lr=1e-4, beta=0.6, steps=200, episode=11, q_scale=1.0, stride=509, limit=256),
}
TAPPED = ["q", "q_pred", "next_q", "next_target_q", "target_q", "td_error", "priority", "p_j", "loss", "indices", "weights", "sampled_p", "mean_p", "max_Q"]
MAX_BYTES = 461784  # the largest fixture of the value family already committed (qrdqn_cartpole.npz)
THIN_LIMIT, ACT_NP_SEED, INIT_SEED = 2048, 7, 5
SCALED = ("l2_a.weight", "l2_a.bias", "l2_v.weight", "l2_v.bias")
CURVE_STEPS, CURVE_CHUNK, CURVE_SEEDS = 12000, 1000, (1, 2, 3)
CURVE_CONFIG = dict(steps=CURVE_STEPS, chunk=CURVE_CHUNK, run_step=CURVE_STEPS, hidden=512, batch=64, lr=1e-4, gamma=0.99, clip_grad_norm=40.0, start=2000, target=500,
                    buffer=50000, lr_decay=True, n_step=3, alpha=0.6, beta=0.6, uniform_sample_prob=1e-3, seq_len=4, n_burn_in=1, zero_padding=True)


def agent_kwargs(c):
    return dict(state_size=c["S"], action_size=c["A"], hidden_size=c["H"], network="r2d2", head="mlp", optim_config={"name": "adam", "lr": c["lr"]}, gamma=0.99,
                buffer_size=256, batch_size=c["B"], clip_grad_norm=40.0, start_train_step=0, target_update_period=10000, lr_decay=False, n_step=c["n"], alpha=0.6,
                beta=c["beta"], uniform_sample_prob=1e-3, seq_len=c["seq"], n_burn_in=c["burn"], zero_padding=c["pad"], epsilon=0.4, run_step=100000, device="cpu")


def recipe_weights(shapes, seed, q_scale):
    """The fixture's starting weights of one network: the recipe's, the last layers of both streams scaled."""
    sd = synth.recipe_state_dict(shapes, seed)
    for k in SCALED:
        sd[k] = np.ascontiguousarray(sd[k] * np.float32(q_scale), dtype=np.float32)
    return sd


def fill_loop(agent, c, act_np_seed=ACT_NP_SEED, fill_seed=FILL_SEED):
    """run_mode's single loop without process(): act -> a synthetic env step -> interact_callback -> memory.store([row]).
    -> (what act() returned per step with the state and done beside it, the emitted rows)."""
    rs = np.random.RandomState(fill_seed)
    np.random.seed(act_np_seed)
    state, trace, rows = rs.randn(1, c["S"]).astype(np.float32), [], []
    for t in range(c["steps"]):
        out = agent.act(state, True)
        nxt = rs.randn(1, c["S"]).astype(np.float32)
        done = (t + 1) % c["episode"] == 0
        tr = {"state": state, "next_state": nxt, "reward": np.asarray([[rs.choice([-1.0, 0.0, 1.0, 0.5])]], np.float32), "done": np.asarray([[done]])}
        tr.update(out)
        trace.append(dict(out, state=state, done=np.asarray(done)))
        row = agent.interact_callback(tr)
        if row:
            rows.append(row)
            agent.memory.store([row])
        state = nxt
    return trace, rows


def target_truth(rec, c):
    """The float64 evaluation of r2d2.py:124-141 on the tapped float32 next_q / next_target_q and the sampled reward / done."""
    from r2d2_truth import fold

    nq, ntq = rec["next_q"].astype(np.float64), rec["next_target_q"].astype(np.float64)
    B, T = nq.shape[:2]
    best = nq.argmax(-1)
    t = ntq[np.arange(B)[:, None], np.arange(T)[None, :], best][..., None]
    return fold(t, rec["reward"].astype(np.float64), rec["done"].astype(np.float64), c["burn"], c["n"], c["seq"], float(np.float32(0.99)))


def gen_fixture(name, out_dir):
    import torch
    from core.agent.r2d2 import R2D2

    c, kw = SPECS[name], agent_kwargs(SPECS[name])
    limit = c.get("limit", THIN_LIMIT)
    keep = lambda v: synth.thin(v, limit, c["stride"])
    out = {}
    torch.manual_seed(INIT_SEED)
    fresh = R2D2(**kw)
    refkit.flat("init_thin/", {k: keep(v) for k, v in refkit.sd_to_np(fresh.network.state_dict()).items()}, out)
    refkit.seed_rngs(3)
    agent = R2D2(**kw)
    shapes = {k: tuple(v.shape) for k, v in agent.network.state_dict().items()}
    with torch.no_grad():
        for i, mod in enumerate((agent.network, agent.target_network)):
            mod.load_state_dict({k: torch.from_numpy(v) for k, v in recipe_weights(shapes, RECIPE_SEED + i, c["q_scale"]).items()})
    for k, v in shapes.items():
        out[f"shape/{k}"] = np.asarray(v, dtype=np.int64)
    agent.memory.first_store = False
    trace, rows = fill_loop(agent, c)
    TRACE = c["episode"] + 3  # the recorded acting trace runs across the first episode end
    assert len(rows) >= c["B"] and sum(int(t["done"]) for t in trace[:TRACE]) >= 1
    for k in trace[0]:
        out[f"trace/{k}"] = np.stack([np.asarray(t[k]) for t in trace[:TRACE]])
    for k in rows[0]:
        out[f"rows/{k}"] = keep(np.concatenate([np.asarray(r[k]).astype(np.float32) for r in rows], 0))
    out["rows/priority64"] = np.concatenate([np.asarray(r["priority"], np.float64).reshape(-1) for r in rows])
    out["rows/padded"] = np.asarray([int(np.asarray(r["action"]).dtype == np.float64) for r in rows])
    out["tree0"] = np.asarray(agent.memory.sum_tree, np.float64).copy()
    markers = {"pre_step": ("self.optimizer.zero_grad", TAPPED + ["action", "reward", "done", "state"]), "step": ("self.optimizer.step()", [])}
    refkit.seed_rngs(42)
    errs = []
    for k in range(2):
        tap = refkit.LineTap(R2D2.learn, markers)
        grads = {}
        tap.on_line["step"] = lambda frame: grads.update(refkit.grads_of(agent.network))
        with tap:
            result = agent.learn()
        rec = dict(tap.records["pre_step"][0])
        state, done = rec.pop("state"), rec["done"]
        if c["pad"]:
            assert (~state[:, 0].any(-1)).any(), f"{name} learn {k}: no zero-padded row in the sampled batch; pick another seed"
        assert done[:, c["burn"]:].any(), f"{name} learn {k}: no row with done inside the columns the trained steps' fold reads"
        top = np.sort(rec["next_q"].astype(np.float64), -1)
        gap, bound = top[..., -1] - top[..., -2], 2.0 * 2.0 ** -24 * np.abs(rec["next_q"]).max()
        assert (gap > bound).all(), f"{name} learn {k}: a near-tie of the two best next actions (gap {gap.min():.3e})"
        t64 = target_truth(rec, c)
        errs.append(float(np.abs(rec["target_q"].astype(np.float64) - t64).max() / np.abs(t64).max()))
        print(name, "learn", k, "max |target_q|", float(np.abs(t64).max()), "ref_target_err", errs[-1])
        p = f"l{k}/"
        refkit.flat(p + "learn/", rec, out)
        refkit.flat(p + "result/", {kk: np.asarray(v) for kk, v in result.items()}, out)
        refkit.flat(p + "grad_thin/", {kk: keep(v) for kk, v in grads.items()}, out)
        for kk, v in grads.items():
            out[f"{p}grad_absmax/{kk}"] = np.abs(v).max()
        out[p + "grad_norm"] = refkit.grad_norm(grads)
        refkit.flat(p + "sd1_thin/", {kk: keep(v) for kk, v in refkit.sd_to_np(agent.network.state_dict()).items()}, out)
        for m in ("exp_avg", "exp_avg_sq"):
            refkit.flat(f"{p}opt1_thin/{m}/", {kk: keep(agent.optimizer.state[pp][m].detach().numpy().copy()) for kk, pp in agent.network.named_parameters()}, out)
        out[p + "tree"] = np.asarray(agent.memory.sum_tree, np.float64).copy()
        out[p + "beta_after"] = np.asarray(agent.beta)
    if c["q_scale"] != 1.0:
        assert max(errs) <= 0.5e-5, f"{name}: the reference's target_q is {max(errs):.2e} of its largest entry from float64; raise q_scale"
    refkit.put_hyper(out, dict(S=c["S"], A=c["A"], H=c["H"], B=c["B"], seq_len=c["seq"], n_burn_in=c["burn"], n_step=c["n"], zero_padding=int(c["pad"]), lr=c["lr"],
                               beta=c["beta"], alpha=0.6, eta=0.9, gamma=0.99, clip_grad_norm=40.0, epsilon=0.4, steps=c["steps"], episode=c["episode"],
                               q_scale=c["q_scale"], thin_stride=c["stride"], thin_limit=limit, trace=TRACE, act_np_seed=ACT_NP_SEED, fill_seed=FILL_SEED,
                               recipe_seed=RECIPE_SEED, init_seed=INIT_SEED, np_seed=42, torch_seed=42, n_rows=len(rows), ref_target_err=max(errs)))
    refkit.save_fixture(out_dir, name, out, cap=MAX_BYTES)


def reference_curve(seed):
    """config.r2d2.cartpole in run_mode's single loop (process only when interact_callback emits a row) on the oracle's CartPole -> mean
    episode length per CURVE_CHUNK env steps."""
    from core.agent.r2d2 import R2D2

    from oracle.dqn_port import make_env

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = R2D2(state_size=4, action_size=2, hidden_size=c["hidden"], network="r2d2", head="mlp", optim_config={"name": "adam", "lr": c["lr"]}, gamma=c["gamma"],
                 buffer_size=c["buffer"], batch_size=c["batch"], clip_grad_norm=c["clip_grad_norm"], start_train_step=c["start"], target_update_period=c["target"],
                 lr_decay=c["lr_decay"], n_step=c["n_step"], alpha=c["alpha"], beta=c["beta"], uniform_sample_prob=c["uniform_sample_prob"], seq_len=c["seq_len"],
                 n_burn_in=c["n_burn_in"], zero_padding=c["zero_padding"], run_step=c["run_step"], device="cpu")
    agent.memory.first_store = False
    env, state = make_env(1000 + seed)
    out, lens, ep = [], [], 0
    for step in range(1, c["steps"] + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"]).reshape(-1))
        tr = {"state": state, "next_state": nxt.astype(np.float32), "reward": rew.reshape(1, 1).astype(np.float64), "done": done.reshape(1, 1)}
        tr.update(a)
        row = agent.interact_callback(tr)
        if row:
            agent.process([row], step)
        state = env.obs().astype(np.float32)
        ep += 1
        if bool(done.reshape(-1)[0]):
            lens.append(ep)
            ep = 0
        if step % c["chunk"] == 0:
            out.append(float(np.mean(lens)) if lens else float(ep))
            lens = []
    return out


def curve_learns(curves):
    """The DQN curve test's criteria (tests/test_learning_curve_gpu.py): starts near random play, and learns."""
    start, end = np.mean([np.mean(x[:2]) for x in curves]), np.mean([np.mean(x[-4:]) for x in curves])
    return bool(start < 40 and end > 4 * start), float(start), float(end)


def gen_curves(out_dir, threads):
    curves = refkit.seeded_curves(reference_curve, CURVE_SEEDS, "r2d2")
    ok, start, end = curve_learns(curves)
    print(f"reference R2D2 episode length {start:.1f} -> {end:.1f}: {'learns' if ok else 'DOES NOT LEARN'} within {CURVE_STEPS} steps by the DQN curve test's criteria", flush=True)
    doc = refkit.curve_doc("tools/gen_golden_r2d2.py --only curves (the unmodified reference R2D2, CPU, scratch copy)", CURVE_SEEDS, threads, reference_learns=ok,
                           start=start, end=end, r2d2_cartpole={"config": CURVE_CONFIG, "metric": "mean episode length per 1000 env steps", "reference": curves})
    refkit.write_curves(os.path.join(out_dir, "curves_reference_r2d2.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=8)
