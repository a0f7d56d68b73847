#!/usr/bin/env python3
"""Golden vectors and the reference learning curves of REINFORCE, from the UNMODIFIED reference agent (core/agent/reinforce.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `learn()` runs, the hooks, the storage helpers and the curve loop are
oracle/refkit.py's; this file holds none of the reference's code.

  tests/golden/reinforce_discrete.npz    S 4, A 3, H 64, lr 3e-3, run_step 1000: TWO CONSECUTIVE learns of different lengths, 37 rows and then 12
                                         (the variable T, Adam step 2, the lr decay between them); perturbed weights, every tensor in full
  tests/golden/reinforce_continuous.npz  continuous_policy, S 5, A 3, H 32; 29 rows and then 50.  Stored actions hold exact +1.0 and -1.0; the
                                         mu layer is scaled up so that some mu_raw lie beyond +-5 (clamped: no gradient) and others inside
  tests/golden/reinforce_nostd.npz       use_standardization False, gamma 1.0, 9 rows
  tests/golden/reinforce_cartpole.npz    config.reinforce.cartpole exactly (H 512, lr 1e-4, gamma 0.99, run_step 100000): ONE real episode of the
                                         oracle's CartPole under the reference's own act(); recipe weights (regenerated from the seed by the
                                         reader), big arrays thinned
  tests/golden/curves_reference_reinforce.json   the oracle's CartPole in single mode, seeds 1-3: mean episode length per `chunk` env steps, at the
                                         smallest budget tried at which the reference's last tenth is at least twice its first on all three seeds
                                         (tests/reinforce_truth.py's CURVE_CONFIG; `search` records what every budget tried gave)

Every transition goes through process([transition], step) as the single-mode loop hands it over: only the last one of an episode is done and
learns.  A learn `l<k>/` holds the stored rows `in/*` with their step numbers, the tapped `ret`, the raw network output `out` (logits, or
mu_raw | log_std_raw) with its retained gradient `d_out`, log_prob, the loss, the raw parameter gradients, the weights and Adam moments after the step
and the lr after the decay.  hyper/thin_limit > 0: arrays larger than that are strided samples (tests/reinforce_truth.py's thin).
A condition the generator asserts on every recorded learn (the row seed -- the env seed of the CartPole episode -- is the first from its start
value up that meets it): the loss is a well-conditioned sum, kappa = sum |log_prob ret| / |sum log_prob ret| <= 64 (`l<k>/kappa`).  The
standardised returns have zero mean, so under a near-uniform policy the terms cancel and the reference's own float32 loss carries a relative
error of about kappa 2^-24 against the exact sum; at kappa 64 that is 3.8e-6, under half of the rtol 1e-5 the tests hold the loss to, so the
recorded loss pins the agent and not the reference's rounding.

Usage:  python tools/gen_golden_reinforce.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 4]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reinforce_truth as D  # noqa: E402  (the recipe weights and the curve configuration are shared with the tests)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import RECIPE_SEED, LineTap, flat, grads_of, sd_to_np  # noqa: E402

SPECS = {
    "reinforce_discrete": dict(S=4, A=3, H=64, cont=False, rows=(37, 12), lr=3e-3, gamma=0.99, standardize=True, run_step=1000, recipe=False, thin_limit=0),
    "reinforce_continuous": dict(S=5, A=3, H=32, cont=True, rows=(29, 50), lr=3e-3, gamma=0.99, standardize=True, run_step=1000, recipe=False, thin_limit=0),
    "reinforce_nostd": dict(S=4, A=3, H=64, cont=False, rows=(9,), lr=3e-3, gamma=1.0, standardize=False, run_step=1000, recipe=False, thin_limit=0),
    "reinforce_cartpole": dict(S=4, A=2, H=512, cont=False, rows=None, lr=1e-4, gamma=0.99, standardize=True, run_step=100000, recipe=True, thin_limit=8192),
}
INIT_SEED, ROW_SEED, PERTURB, MU_SCALE, ENV_SEED, ACT_SEED, MAX_KAPPA = 11, 23, 0.1, 15.0, 1003, 5, 64.0


def agent_kwargs(spec):
    return dict(state_size=spec["S"], action_size=spec["A"], hidden_size=spec["H"], network="continuous_policy" if spec["cont"] else "discrete_policy", head="mlp",
                optim_config={"name": "adam", "lr": spec["lr"]}, gamma=spec["gamma"], use_standardization=spec["standardize"], run_step=spec["run_step"], lr_decay=True,
                device="cpu")


def synthetic_rows(rs, T, S, A, cont):
    """One synthetic episode of T one-row transitions: only the last is done.  Continuous actions hold exact +1.0 and -1.0."""
    out = []
    for t in range(T):
        action = np.tanh(1.5 * rs.randn(1, A)).astype(np.float32) if cont else rs.randint(0, A, size=(1, 1))
        if cont and t == 1:
            action[0, 0] = 1.0
        if cont and t == 2:
            action[0, A - 1] = -1.0
        out.append({"state": rs.randn(1, S).astype(np.float32), "action": action, "reward": rs.choice([-1.0, 0.0, 1.0, 0.5], size=(1, 1)),
                    "next_state": rs.randn(1, S).astype(np.float32), "done": np.asarray([[t == T - 1]])})
    return out


def cartpole_rows(agent, env_seed):
    """One real episode of the oracle's CartPole under the reference agent's own act(training=True)."""
    from oracle.dqn_port import make_env

    refkit.seed_rngs(ACT_SEED)
    env, state = make_env(env_seed)
    out = []
    while True:
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"]).reshape(-1))
        tr = {"state": state, "next_state": nxt.astype(np.float32), "reward": rew.reshape(1, 1).astype(np.float64), "done": done.reshape(1, 1)}
        tr.update(a)
        out.append(tr)
        state = env.obs().astype(np.float32)
        if bool(done.reshape(-1)[0]):
            return out


def record_learn(agent, spec, trs, steps, keep):
    """process([transition], step) for every row of one episode; the last one learns under the line tap -> flat dict."""
    for tr, step in zip(trs[:-1], steps[:-1]):
        assert agent.process([tr], step) == {}, "only the episode's last transition learns"
    heads = {"mu": agent.network.mu, "log_std": agent.network.log_std} if spec["cont"] else {"pi": agent.network.pi}
    outs, hooks = refkit.retaining_hooks(heads)
    markers = {"loss": ("(log_prob * ret).mean()", ["ret", "log_prob"]), "step": ("self.optimizer.step()", [])}
    tap = LineTap(type(agent).learn, markers)
    got = {}

    def on_step(frame):
        got["grads"] = grads_of(agent.network)
        got["heads"] = refkit.last_outputs(outs)

    tap.on_line["step"] = on_step
    with tap:
        result = agent.process([trs[-1]], steps[-1])
    for h in hooks:
        h.remove()
    assert all(len(v) == 1 for v in outs.values()) and set(result) == {"loss"}
    T = len(trs)
    rec = tap.records["loss"][0]
    h = got["heads"]
    out = {"steps": np.asarray(steps, np.int64), "ret": rec["ret"].reshape(-1), "log_prob": rec["log_prob"], "loss": np.asarray(result["loss"], np.float32)}
    if spec["cont"]:
        out["out"], out["d_out"] = np.concatenate([h["mu"], h["log_std"]], 1), np.concatenate([h["d_mu"], h["d_log_std"]], 1)
    else:
        out["out"], out["d_out"] = h["pi"], h["d_pi"]
    assert out["out"].shape[0] == T and out["ret"].shape == (T,)
    for c in D.COLUMNS:
        out[f"in/{c}"] = np.concatenate([tr[c] for tr in trs], 0)
    flat("grad/", {k: keep(v) for k, v in got["grads"].items()}, out)
    for k, v in got["grads"].items():
        out[f"grad_absmax/{k}"] = np.abs(v).max()
    flat("sd1/", {k: keep(v) for k, v in sd_to_np(agent.network.state_dict()).items()}, out)
    for k, p in agent.network.named_parameters():
        st = agent.optimizer.state[p]
        out[f"opt/exp_avg/{k}"], out[f"opt/exp_avg_sq/{k}"] = keep(st["exp_avg"].detach().numpy().copy()), keep(st["exp_avg_sq"].detach().numpy().copy())
        out["opt/step"] = np.asarray(int(float(st["step"])))
    out["lr"] = np.asarray(agent.optimizer.param_groups[0]["lr"], np.float64)
    terms = rec["log_prob"].astype(np.float64).reshape(T, -1) * rec["ret"].astype(np.float64).reshape(T, 1)
    out["kappa"] = np.asarray(np.abs(terms).sum() / abs(terms.sum()))
    return out


def try_fixture(name, offset):
    """-> (the fixture with its row seed / env seed moved up by `offset`, whether every learn meets the condition)"""
    import torch
    from core.agent.reinforce import REINFORCE

    spec = SPECS[name]
    S, A, recipe, limit = spec["S"], spec["A"], spec["recipe"], spec["thin_limit"]
    keep = refkit.keeper(limit)
    refkit.seed_rngs(INIT_SEED)
    agent = REINFORCE(**agent_kwargs(spec))
    agent.memory.first_store = False
    with torch.no_grad():
        if recipe:
            rec = D.recipe_weights({k: tuple(v.shape) for k, v in agent.network.state_dict().items()}, RECIPE_SEED, synth)
            for k, p in agent.network.named_parameters():
                p.copy_(torch.from_numpy(rec[k]))
        else:  # perturb so that pi is not ~uniform (the policy gain is 0.01)
            for p in agent.network.parameters():
                p.add_(PERTURB * torch.randn_like(p))
            if spec["cont"]:
                agent.network.mu.weight.mul_(MU_SCALE)  # mu_raw on both sides of +-5
    out = {}
    sd0 = sd_to_np(agent.network.state_dict())
    if not recipe:
        flat("sd0/", sd0, out)
    for k, v in sd0.items():
        out[f"shape/{k}"] = np.asarray(v.shape)
    rs = np.random.RandomState(ROW_SEED + offset)
    step, rows, ok = 0, [], True
    episodes = [None] if spec["rows"] is None else spec["rows"]
    for k, T in enumerate(episodes):
        trs = cartpole_rows(agent, ENV_SEED + offset) if T is None else synthetic_rows(rs, T, S, A, spec["cont"])
        steps = list(range(step + 1, step + len(trs) + 1))
        step = steps[-1]
        rows.append(len(trs))
        rec = record_learn(agent, spec, trs, steps, keep)
        if spec["cont"]:
            mu_raw = rec["out"][:, :A]
            assert (np.abs(mu_raw) > 5.0).any() and (np.abs(mu_raw) < 5.0).any(), "mu_raw on both sides of the clamp"
            assert (rec["in/action"] == 1.0).any() and (rec["in/action"] == -1.0).any(), "saturated actions"
            assert np.isfinite(rec["d_out"]).all() and np.isfinite(rec["loss"])
        ok = ok and float(rec["kappa"]) <= MAX_KAPPA
        flat(f"l{k}/", rec, out)
        print(name, f"l{k}", len(trs), "rows, loss", float(rec["loss"]), "lr", float(rec["lr"]), "kappa", float(rec["kappa"]))
    refkit.put_hyper(out, dict(S=S, A=A, H=spec["H"], lr=spec["lr"], gamma=spec["gamma"], standardize=int(spec["standardize"]), cont=int(spec["cont"]), run_step=spec["run_step"],
                               recipe=int(recipe), recipe_seed=RECIPE_SEED, thin_limit=limit, init_seed=INIT_SEED, row_seed=ROW_SEED + offset, perturb=PERTURB, mu_scale=MU_SCALE,
                               env_seed=ENV_SEED + offset, act_seed=ACT_SEED, max_kappa=MAX_KAPPA, rows=np.asarray(rows, np.int64)))
    return out, ok


def gen_fixture(name, out_dir):
    for offset in range(64):
        out, ok = try_fixture(name, offset)
        if ok:
            break
        print(name, f"seed offset {offset}: a learn's loss is an ill-conditioned sum, next seed")
    else:
        raise SystemExit(f"{name}: no seed meets the condition")
    refkit.save_fixture(out_dir, name, out, cap=1 << 20, note=f"seed offset {offset}")


def reference_curve(seed, c):
    from core.agent.reinforce import REINFORCE

    refkit.seed_rngs(seed)
    agent = REINFORCE(run_step=c["run_step"], device="cpu", **c["agent"])
    agent.memory.first_store = False
    return refkit.value_cartpole_curve(agent, seed, c["steps"], c["chunk"])


def gen_curves(out_dir, threads):
    """The budget search the fixture's configuration came from: lr 1e-3, 20000 steps, then larger budgets up to 30000; the first at which the
    last tenth is at least twice the first tenth on all three seeds is kept (the last one tried if none is)."""
    c0 = D.CURVE_CONFIG
    search, kept = [], None
    for steps in sorted({c0["steps"], 25000, 30000}):
        if steps < c0["steps"]:
            continue
        c = dict(c0, steps=steps, run_step=steps)
        curves = refkit.seeded_curves(lambda s: reference_curve(s, c), c["seeds"], f"reinforce {steps}")
        tenths = [D.curve_tenths(v) for v in curves]
        ok = all(last >= 2.0 * first for first, last in tenths)
        search.append({"steps": steps, "lr": c["agent"]["optim_config"]["lr"], "first_last_tenths": tenths, "accepted": ok})
        kept = (c, curves)
        print("first / last tenth:", tenths, "accepted" if ok else "not accepted")
        if ok:
            break
    c, curves = kept
    doc = refkit.curve_doc("tools/gen_golden_reinforce.py --only curves (the unmodified reference REINFORCE, CPU, scratch copy)", c["seeds"], threads, config=c,
                           metric=f"mean episode length per {c['chunk']} env steps (single mode)", search=search, accepted=bool(search[-1]["accepted"]))
    doc["reinforce_cartpole"] = {"reference": curves}
    refkit.write_curves(os.path.join(out_dir, "curves_reference_reinforce.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=4)
