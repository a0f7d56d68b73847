#!/usr/bin/env python3
"""Golden vectors and the reference learning curve of Rainbow-IQN, from the UNMODIFIED reference agent (core/agent/rainbow_iqn.py on
core/network/rainbow_iqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `RainbowIQN.learn()` runs on the CPU and the value family's recorder are
oracle/refkit.py's; this file holds none of the reference's code.

A learn() draws on torch's CPU generator in this order: per forward (online(s), online(s'), target(s')) the tau draw of make_embed, then the
NoisyNet draws of the four layers a1, v1, a2, v2 (utils.py:58-60, 75-76).  Both are recorded while they happen -- make_embed wrapped as
tools/gen_golden_iqn.py does, torch.randn wrapped for the duration of the learn() -- and stored as learn/tau [3][B][N] and learn/noise
[3][noise_len], a noise set being the concatenation of a forward's draws in draw order, each flattened (the layout ops.RainbowIQNNet takes).

The weights come from synth.recipe_state_dict (seed and seed + 1 for online and target); tensors over thin_limit entries are stored as
every thin_stride-th entry (THIN).  The
priorities in front of the first learn() are RandomState(FILL_SEED + 1).rand() ** 2 + 0.01 per stored window, as oracle/gen_golden.py sets
them for Rainbow; `riqn` raises three windows -- the first with a done at its first step only, at a middle step only, at its last step
only -- to BOOST so that the sampled batch has each (asserted).  Every fixture records two consecutive learns (learn/, learn2/), each
after np.random.seed / torch.manual_seed (42).

  tests/golden/riqn.npz            S 4, A 3, H 64, E 8, N 8, B 8, n_step 3, factorized noise, Adam 1e-3
  tests/golden/riqn_odd.npz        S 8, A 5, H 36, E 5, N 7, B 6, n_step 2, independent noise
  tests/golden/riqn_cartpole.npz   config.rainbow_iqn.cartpole exactly (S 4, A 2, H 512, E 64, N 64, B 32, n_step 3, alpha 0.6, beta 0.4,
                                   uniform_sample_prob 1e-3, factorized noise, Adam 1e-4, eps 1e-2 / 32)
  tests/golden/curves_reference_riqn.json   the reduced agent of CURVE_CONFIG in refkit.value_cartpole_curve (--only curves)

Usage:  python tools/gen_golden_riqn.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 8]
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
    "riqn": dict(state_size=4, action_size=3, hidden_size=64, embedding_dim=8, num_sample=8, batch_size=8, n_step=3, noise_type="factorized",
                 alpha=0.5, beta=0.4, uniform_sample_prob=0.05, optim_config={"name": "adam", "lr": 1e-3}),
    "riqn_odd": dict(state_size=8, action_size=5, hidden_size=36, embedding_dim=5, num_sample=7, batch_size=6, n_step=2, noise_type="independent",
                     alpha=0.5, beta=0.4, uniform_sample_prob=0.05, optim_config={"name": "adam", "lr": 1e-3}),
    "riqn_cartpole": dict(state_size=4, action_size=2, hidden_size=512, embedding_dim=64, num_sample=64, batch_size=32, n_step=3, noise_type="factorized",
                          alpha=0.6, beta=0.4, uniform_sample_prob=1e-3, optim_config={"name": "adam", "lr": 1e-4, "eps": 1e-2 / 32}),
}
TAPPED = ["logit", "logit_next", "logit_target", "q_next", "max_a", "theta_pred", "theta_target", "p_j", "loss", "weights", "indices", "state", "action", "reward",
          "next_state", "done"]
MAX_BYTES = 1 << 20  # what a committed file may have; two recorded learns of 26 tensors each
THIN = {"riqn": (1024, 7), "riqn_odd": (1024, 7), "riqn_cartpole": (4096, 509)}  # (largest tensor stored whole, stride of the sample of a larger one)
BOOST = 40.0
FILL = 200


def thinner(name):
    limit, stride = THIN[name]
    return lambda a: synth.thin(a, limit=limit, stride=stride)


CURVE_STEPS, CURVE_RUN_STEP, CURVE_CHUNK, CURVE_SEEDS = 12000, 15000, 1000, (1, 2, 3)
# config.rainbow_iqn.cartpole with hidden_size 128 and num_sample 32: the reduction keeps the reference's CPU run to minutes
CURVE_CONFIG = dict(steps=CURVE_STEPS, chunk=CURVE_CHUNK, run_step=CURVE_RUN_STEP, hidden_size=128, batch=32, num_sample=32, embedding_dim=64, sample_min=0.0,
                    sample_max=1.0, lr=1e-4, eps=1e-2 / 32, gamma=0.99, start=2000, target=1000, buffer=50000, lr_decay=True, n_step=3, alpha=0.6, beta=0.4,
                    learn_period=2, uniform_sample_prob=1e-3, noise_type="factorized")


def agent_kwargs(spec):
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, learn_period=1, network="rainbow_iqn", head="mlp",
              device="cpu")
    kw.update(spec)
    return kw


@contextlib.contextmanager
def recording_draws(taus, normals):
    """Every tau draw of the network class's make_embed and every torch.randn, in call order, while the block runs."""
    import torch
    from core.network.rainbow_iqn import RainbowIQN as Net

    inner_embed, inner_randn = Net.make_embed, torch.randn

    def embed(self, x, tau_min, tau_max):
        res = inner_embed(self, x, tau_min, tau_max)
        taus.append(res[1].detach().numpy().copy())
        return res

    def randn(*a, **k):
        res = inner_randn(*a, **k)
        normals.append(res.detach().numpy().copy().reshape(-1))
        return res

    Net.make_embed, torch.randn = embed, randn
    try:
        yield
    finally:
        Net.make_embed, torch.randn = inner_embed, inner_randn


def draws_entry(taus, normals, kw):
    """learn/tau [3][B][N] and learn/noise [3][noise_len] in call order, in front of the other learn/ entries."""
    B, N, H, A = kw["batch_size"], kw["num_sample"], kw["hidden_size"], kw["action_size"]
    assert len(taus) == 3 and all(t.shape == (B, N, 1) for t in taus)
    assert len(normals) == 24  # three forwards x four layers x two draws
    sets = [np.concatenate(normals[8 * f : 8 * f + 8]) for f in range(3)]
    want = 2 * (H * H + H) + H * A + A + H + 1 if kw["noise_type"] == "independent" else 6 * H + A + 1
    assert all(s.size == want for s in sets)
    return {"learn/tau": np.stack([t.reshape(B, N) for t in taus]), "learn/noise": np.stack(sets).astype(np.float32)}


def set_priorities(agent, name):
    rng = np.random.RandomState(FILL_SEED + 1)
    mem = agent.memory
    for leaf in range(mem.size):
        mem.update_priority(float(np.float32(rng.rand() ** 2 + 0.01)), leaf + mem.first_leaf_index)
    if name != "riqn":
        return
    n = agent.n_step
    want = {0: None, n // 2: None, n - 1: None}
    for slot in range(mem.size):
        d = np.asarray(mem.buffer[slot]["done"]).reshape(-1).astype(bool)
        if d.sum() == 1 and int(np.argmax(d)) in want and want[int(np.argmax(d))] is None:
            want[int(np.argmax(d))] = slot
    assert all(v is not None for v in want.values()), want
    for slot in want.values():
        mem.update_priority(BOOST, slot + mem.first_leaf_index)


def record_learn(agent, kw, out, prefix):
    """One learn() under the tap -> `out[prefix + ...]`; -> (the step for refkit.store_step, the result)."""
    rec, taus, normals = {}, [], []
    rec["tree0"], rec["maxp0"], rec["tree_index0"] = agent.memory.sum_tree.copy(), np.asarray(agent.memory.max_priority), np.asarray(agent.memory.tree_index)
    markers = {"loss_b": ("p_j = torch.pow", []), "pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])}
    # in front of the line that forms the priorities, `loss` is still the per-sample loss [B]
    per_sample = lambda frame: {"loss_b": frame.f_locals["loss"].detach().numpy().copy()}
    step, result = refkit.record_value_learn(agent, markers, rec, watch="logit", at="loss_b", name="logit", extra=per_sample,
                                             around=recording_draws(taus, normals), first=lambda: draws_entry(taus, normals, kw))
    rec["tree1"], rec["maxp1"] = agent.memory.sum_tree.copy(), np.asarray(agent.memory.max_priority)
    for k, v in rec.items():
        out[(prefix + k[len("learn/"):]) if k.startswith("learn/") else (k if prefix == "learn/" else prefix + k)] = v
    return step, result


def gen_fixture(name, out_dir):
    from core.agent.rainbow_iqn import RainbowIQN

    kw = agent_kwargs(SPECS[name])
    B, N, A, n = kw["batch_size"], kw["num_sample"], kw["action_size"], kw["n_step"]
    agent, out = refkit.value_agent(RainbowIQN, kw, recipe=True, fill=FILL)
    assert out["buf_reward"].shape == (FILL - n + 1, n, 1) and out["buf_done"].shape == (FILL - n + 1, n, 1)
    set_priorities(agent, name)
    step, result = record_learn(agent, kw, out, "learn/")
    assert out["learn/logit"].shape == (B, N, A) and out["learn/d_logit"].shape == (B, N, A) and out["learn/loss_b"].shape == (B,)
    if name == "riqn":
        d = out["learn/done"].reshape(B, n).astype(bool)
        single = d.sum(1) == 1
        assert {0, n // 2, n - 1} <= set(np.argmax(d[single], 1).tolist()), "the sampled batch lacks a done at the first, a middle or the last step of a window"
    out["fill"], out["fill_seed"], out["recipe_seed"] = np.asarray(FILL), np.asarray(FILL_SEED), np.asarray(RECIPE_SEED)
    out["thin_limit"], out["thin_stride"] = (np.asarray(v) for v in THIN[name])
    thin = thinner(name)
    refkit.store_step(out, agent, *step, thin=thin, moments=("exp_avg", "exp_avg_sq"), sd0_min=THIN[name][0])
    refkit.put_result(out, result)
    # the second learn(): the weights, moments and tree the first one left
    out2 = {}
    step2, result2 = record_learn(agent, kw, out2, "learn2/")
    refkit.store_step(out2, agent, *step2, thin=thin, moments=("exp_avg", "exp_avg_sq"), sd0_min=1 << 62)
    out.update({(k if k.startswith("learn2/") else "learn2/" + k): v for k, v in out2.items()})
    for k, v in result2.items():
        out[f"learn2/result/{k}"] = np.asarray(v)
    shapes = {k: tuple(v.shape) for k, v in agent.network.state_dict().items()}
    for k, v in shapes.items():
        out[f"shape/{k}"] = np.asarray(v, dtype=np.int64)
    hyper = dict(gamma=0.99, lr=kw["optim_config"]["lr"], B=B, S=kw["state_size"], A=A, H=kw["hidden_size"], E=kw["embedding_dim"], N=N, n_step=n, alpha=kw["alpha"],
                 beta=kw["beta"], uniform_sample_prob=kw["uniform_sample_prob"], noise_type=kw["noise_type"], sample_min=0.0, sample_max=1.0, np_seed=42, torch_seed=42)
    hyper.update({f"optim_{k}": v for k, v in kw["optim_config"].items() if isinstance(v, (int, float, bool))})
    refkit.put_hyper(out, hyper)
    refkit.save_fixture(out_dir, name, out, cap=MAX_BYTES)


class Windowed:
    """The agent as the single-mode loop drives it (run_mode.py:68-91): every env step goes through interact_callback, and only an assembled
    n-step window reaches process().  refkit.value_cartpole_curve hands process() the raw steps."""

    def __init__(self, agent):
        self.agent = agent

    def act(self, state, training=True):
        return self.agent.act(state, training)

    def process(self, transitions, step):
        windows = [w for w in (self.agent.interact_callback(t) for t in transitions) if w]
        return self.agent.process(windows, step) if windows else {}


def reference_curve(seed):
    """The reduced config.rainbow_iqn.cartpole in refkit.value_cartpole_curve, the loop of tests/test_learning_curve_gpu.py::_dqn_curve."""
    from core.agent.rainbow_iqn import RainbowIQN

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = RainbowIQN(state_size=4, action_size=2, hidden_size=c["hidden_size"], network="rainbow_iqn", num_sample=c["num_sample"], embedding_dim=c["embedding_dim"],
                       sample_min=c["sample_min"], sample_max=c["sample_max"], optim_config={"name": "adam", "lr": c["lr"], "eps": c["eps"]}, gamma=c["gamma"],
                       buffer_size=c["buffer"], batch_size=c["batch"], start_train_step=c["start"], target_update_period=c["target"], lr_decay=c["lr_decay"],
                       run_step=c["run_step"], n_step=c["n_step"], alpha=c["alpha"], beta=c["beta"], learn_period=c["learn_period"],
                       uniform_sample_prob=c["uniform_sample_prob"], noise_type=c["noise_type"], device="cpu")
    return refkit.value_cartpole_curve(Windowed(agent), seed, c["steps"], c["chunk"])


def curve_learns(curves):
    """The reference's side of the IQN curve test's criteria: starts near random play, and learns."""
    start, end = np.mean([np.mean(x[:2]) for x in curves]), np.mean([np.mean(x[-4:]) for x in curves])
    return bool(start < 40 and end > 4 * start), float(start), float(end)


def gen_curves(out_dir, threads):
    curves = refkit.seeded_curves(reference_curve, CURVE_SEEDS, "riqn")
    ok, start, end = curve_learns(curves)
    print(f"reference Rainbow-IQN episode length {start:.1f} -> {end:.1f}: {'learns' if ok else 'DOES NOT LEARN'} by the IQN curve test's criteria", flush=True)
    doc = refkit.curve_doc("tools/gen_golden_riqn.py --only curves (the unmodified reference Rainbow-IQN, CPU, scratch copy)", CURVE_SEEDS, threads, reference_learns=ok,
                           riqn_cartpole={"config": CURVE_CONFIG, "metric": "mean episode length per 1000 env steps", "reference": curves})
    refkit.write_curves(os.path.join(out_dir, "curves_reference_riqn.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=8, default="fixtures")
