#!/usr/bin/env python3
"""Golden vectors and the reference learning curve of IQN, from the UNMODIFIED reference agent (core/agent/iqn.py, core/network/iqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `IQN.learn()` runs and the value family's recorder are oracle/refkit.py's;
this file holds none of the reference's code.  The three tau
draws of a learn() (online(s), online(s'), target(s'), in that order) are recorded by wrapping the network class's make_embed at run time.

The reference builds its network without hidden_size (agent/iqn.py:44-49), so it is 512 wide in every fixture: the weights come from
synth.recipe_state_dict (seed and seed + 1 for online and target) and the big tensors are stored thinned, as mdqn_cartpole.npz does.

  tests/golden/iqn.npz            S 4, A 3, E 16, N 8, B 32, Adam 1e-3
  tests/golden/iqn_odd.npz        S 4, A 5, E 10, N 33, B 7
  tests/golden/iqn_cartpole.npz   config.iqn.cartpole exactly (A 2, E 64, N 64, B 32, Adam 1e-4, eps 1e-2 / 32)
  tests/golden/curves_reference_iqn.json   config.iqn.cartpole in the single-mode loop of tests/test_learning_curve_gpu.py::_dqn_curve

Usage:  python tools/gen_golden_iqn.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 8]
"""
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED  # noqa: E402

SPECS = {
    "iqn": dict(state_size=4, action_size=3, embedding_dim=16, num_sample=8, batch_size=32, optim_config={"name": "adam", "lr": 1e-3}),
    "iqn_odd": dict(state_size=4, action_size=5, embedding_dim=10, num_sample=33, batch_size=7, optim_config={"name": "adam", "lr": 1e-3}),
    "iqn_cartpole": dict(state_size=4, action_size=2, embedding_dim=64, num_sample=64, batch_size=32, optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}),
}
TAPPED = ["logit", "logit_next", "logit_target", "q_next", "max_a", "theta_pred", "theta_target", "loss", "state", "action", "reward", "next_state", "done"]
MAX_BYTES = 461784  # the largest fixture of this family already committed (qrdqn_cartpole.npz)
THIN_STRIDE = 127    # six 512-wide layers x (gradient, weights, two moments): synth.thin's default stride of 61 does not fit MAX_BYTES


def thin(a):
    return synth.thin(a, stride=THIN_STRIDE)


# the initial weights come back from the recipe: only the three biggest tensors' samples are stored, to pin the regeneration
LAYOUT = dict(thin=thin, moments=("exp_avg", "exp_avg_sq"), sd0_min=8192)
CURVE_STEPS, CURVE_RUN_STEP, CURVE_CHUNK, CURVE_SEEDS = 12000, 15000, 1000, (1, 2, 3)
CURVE_CONFIG = dict(steps=CURVE_STEPS, chunk=CURVE_CHUNK, run_step=CURVE_RUN_STEP, batch=32, num_sample=64, embedding_dim=64, sample_min=0.0, sample_max=1.0,
                    lr=1e-4, eps=1e-2 / 32, gamma=0.99, epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


def near_tie_bound(logit_next):
    """[B, N, A] -> (gap [B] of the two best means over N, bound [B]): "near" as tests/test_qrdqn_gpu.py has it (gap <= 2 N 2^-24 max |.|)."""
    z = np.asarray(logit_next, dtype=np.float64)
    B, N, A = z.shape
    q = z.mean(1)
    top = np.sort(q, -1)
    gap = top[:, -1] - top[:, -2] if A > 1 else np.full(B, np.inf)
    return gap, 2.0 * N * 2.0 ** -24 * np.abs(z).reshape(B, -1).max(-1)


def agent_kwargs(spec):
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu")
    kw.update(spec)
    return kw


@contextlib.contextmanager
def recording_taus(taus):
    """Every tau draw of the network class's make_embed, in call order, while the block runs."""
    from core.network.iqn import IQN as IQNNet

    inner = IQNNet.make_embed

    def recording(self, x, tau_min, tau_max):
        res = inner(self, x, tau_min, tau_max)
        taus.append(res[1].detach().numpy().copy())
        return res

    IQNNet.make_embed = recording
    try:
        yield
    finally:
        IQNNet.make_embed = inner


def tau_entry(taus, kw):
    """learn/tau [draws][B][N] in call order, in front of the other learn/ entries."""
    B, N = kw["batch_size"], kw["num_sample"]
    assert all(t.shape == (B, N, 1) for t in taus)
    return {"learn/tau": np.stack([t.reshape(B, N) for t in taus])}


def finish(out_dir, name, out, agent, kw, step, result, note="", **more_hyper):
    """What IQN's and M-IQN's fixtures share after the recorded learn(): the recipe's seeds, the thinned step, the shapes, hyper/* and the cap."""
    B, N, A = kw["batch_size"], kw["num_sample"], kw["action_size"]
    assert out["learn/logit"].shape == (B, N, A) and out["learn/d_logit"].shape == (B, N, A)
    out["fill"], out["fill_seed"], out["recipe_seed"], out["thin_stride"] = np.asarray(200), np.asarray(FILL_SEED), np.asarray(RECIPE_SEED), np.asarray(THIN_STRIDE)
    refkit.store_step(out, agent, *step, **LAYOUT)
    shapes = {k: tuple(v.shape) for k, v in agent.network.state_dict().items()}
    for k, v in shapes.items():
        out[f"shape/{k}"] = np.asarray(v, dtype=np.int64)
    refkit.put_result(out, result)
    hyper = dict(gamma=0.99, lr=kw["optim_config"]["lr"], B=B, S=kw["state_size"], A=A, H=shapes["l1.weight"][0], E=kw["embedding_dim"], N=N, sample_min=0.0, sample_max=1.0,
                 **more_hyper, np_seed=42, torch_seed=42)
    hyper.update({f"optim_{k}": v for k, v in kw["optim_config"].items() if isinstance(v, (int, float, bool))})
    refkit.put_hyper(out, hyper)
    refkit.save_fixture(out_dir, name, out, cap=MAX_BYTES, note=note)


def gen_fixture(name, out_dir):
    from core.agent.iqn import IQN

    kw = agent_kwargs(SPECS[name])
    agent, out = refkit.value_agent(IQN, kw, recipe=True)
    taus = []
    markers = {"pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])}
    step, result = refkit.record_value_learn(agent, markers, out, watch="logit", name="logit", around=recording_taus(taus), first=lambda: tau_entry(taus, kw))
    assert len(taus) == 3  # online(s), online(s'), target(s')
    gap, bound = near_tie_bound(out["learn/logit_next"])
    assert (gap > bound).all(), f"{name}: a row with a near-tie of the two best next actions (gap {gap.min():.3e}); pick another fill seed"
    finish(out_dir, name, out, agent, kw, step, result)


def reference_curve(seed):
    """config.iqn.cartpole in refkit.value_cartpole_curve, the loop of tests/test_learning_curve_gpu.py::_dqn_curve."""
    from core.agent.iqn import IQN

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = IQN(state_size=4, action_size=2, network="iqn", num_sample=c["num_sample"], embedding_dim=c["embedding_dim"], sample_min=c["sample_min"],
                sample_max=c["sample_max"], optim_config={"name": "adam", "lr": c["lr"], "eps": c["eps"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"],
                epsilon_min=c["epsilon_min"], explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"], start_train_step=c["start"],
                target_update_period=c["target"], lr_decay=c["lr_decay"], run_step=c["run_step"], device="cpu")
    return refkit.value_cartpole_curve(agent, seed, c["steps"], c["chunk"])


def curve_learns(curves):
    """The reference's side of the DQN curve test's criteria (tests/test_learning_curve_gpu.py): starts near random play, and learns."""
    start, end = np.mean([np.mean(x[:2]) for x in curves]), np.mean([np.mean(x[-4:]) for x in curves])
    return bool(start < 40 and end > 4 * start), float(start), float(end)


def gen_curves(out_dir, threads):
    curves = refkit.seeded_curves(reference_curve, CURVE_SEEDS, "iqn")
    ok, start, end = curve_learns(curves)
    print(f"reference IQN episode length {start:.1f} -> {end:.1f}: {'learns' if ok else 'DOES NOT LEARN'} by the DQN curve test's criteria", flush=True)
    doc = refkit.curve_doc("tools/gen_golden_iqn.py --only curves (the unmodified reference IQN, CPU, scratch copy)", CURVE_SEEDS, threads, reference_learns=ok,
                           iqn_cartpole={"config": CURVE_CONFIG, "metric": "mean episode length per 1000 env steps", "reference": curves})
    refkit.write_curves(os.path.join(out_dir, "curves_reference_iqn.json"), doc)
    assert ok, "the reference curve does not show learning within these steps: say in DESIGN.md which assertions the curve test keeps"


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=8)
