#!/usr/bin/env python3
"""Golden vectors and the reference learning curve of Munchausen DQN, from the UNMODIFIED reference agent (core/agent/m_dqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `M_DQN.learn()` runs and the value family's recorder are oracle/refkit.py's;
this file holds none of the reference's code.

  tests/golden/mdqn.npz            S 4, A 3, H 32, B 32, discrete_q_network, Adam 1e-3, perturbed online and target weights: every tensor stored
  tests/golden/mdqn_odd.npz        S 4, A 5, H 64, B 7, network "dueling"
  tests/golden/mdqn_cartpole.npz   config.m_dqn.cartpole exactly (H 512, B 32, Adam 1e-4, alpha 0.9, tau 0.03, l_0 -1): recipe weights, thinned
  tests/golden/curves_reference_mdqn.json   config.m_dqn.cartpole in the single-mode loop of tests/test_learning_curve_gpu.py::_dqn_curve

Usage:  python tools/gen_golden_mdqn.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 8]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED  # noqa: E402

M_HYPER = dict(alpha=0.9, tau=0.03, l_0=-1)
SPECS = {
    "mdqn": dict(state_size=4, action_size=3, hidden_size=32, batch_size=32, network="discrete_q_network", optim_config={"name": "adam", "lr": 1e-3}, recipe=False),
    "mdqn_odd": dict(state_size=4, action_size=5, hidden_size=64, batch_size=7, network="dueling", optim_config={"name": "adam", "lr": 1e-3}, recipe=False),
    "mdqn_cartpole": dict(state_size=4, action_size=2, hidden_size=512, batch_size=32, network="discrete_q_network", optim_config={"name": "adam", "lr": 1e-4},
                          recipe=True),
}
# locals of M_DQN.learn in front of optimizer.zero_grad: `q` there is the TAKEN q [B, 1]; network(state) itself is kept by the recorder's forward hook (q_all)
TAPPED = ["q", "next_target_q", "target_q", "clipped_log_policy", "munchausen_term", "maximum_entropy_term", "loss", "state", "action", "reward", "next_state", "done"]

CURVE_STEPS, CURVE_RUN_STEP, CURVE_CHUNK, CURVE_SEEDS = 12000, 15000, 1000, (1, 2, 3)
CURVE_CONFIG = dict(steps=CURVE_STEPS, chunk=CURVE_CHUNK, run_step=CURVE_RUN_STEP, hidden=512, batch=32, alpha=0.9, tau=0.03, l_0=-1, lr=1e-4, gamma=0.99,
                    epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


MARKERS = {"pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])}


def gen_fixture(name, out_dir):
    import torch
    from core.agent.m_dqn import M_DQN

    spec = dict(SPECS[name])
    recipe = spec.pop("recipe")
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu")
    kw.update(spec)
    kw.update(M_HYPER)
    agent, out = refkit.value_agent(M_DQN, kw, recipe)

    def target_on_state(frame):  # the Munchausen term needs the target network on `state` too
        with torch.no_grad():
            return {"target_q_state": agent.target_network(frame.f_locals["state"]).detach().numpy().copy()}

    step, result = refkit.record_value_learn(agent, MARKERS, out, extra=target_on_state)
    assert out["learn/q_all"].shape == (kw["batch_size"], kw["action_size"])
    if recipe:
        out["fill"], out["fill_seed"], out["recipe_seed"] = np.asarray(200), np.asarray(FILL_SEED), np.asarray(RECIPE_SEED)
    refkit.store_step(out, agent, *step, thin=synth.thin if recipe else None, moments=("exp_avg", "exp_avg_sq") if recipe else ())
    refkit.put_result(out, result)
    hyper = dict(gamma=0.99, lr=kw["optim_config"]["lr"], B=kw["batch_size"], S=kw["state_size"], A=kw["action_size"], H=kw["hidden_size"], alpha=M_HYPER["alpha"],
                 m_tau=M_HYPER["tau"], l_0=M_HYPER["l_0"], np_seed=42, torch_seed=42)
    hyper.update({f"optim_{k}": v for k, v in kw["optim_config"].items() if isinstance(v, (int, float, bool))})
    refkit.put_hyper(out, hyper)
    out["hyper/network"] = np.asarray(kw["network"])
    refkit.save_fixture(out_dir, name, out)


def reference_curve(seed):
    """config.m_dqn.cartpole in refkit.value_cartpole_curve, the loop of tests/test_learning_curve_gpu.py::_dqn_curve."""
    from core.agent.m_dqn import M_DQN

    c = CURVE_CONFIG
    refkit.seed_rngs(seed)
    agent = M_DQN(state_size=4, action_size=2, hidden_size=c["hidden"], network="discrete_q_network", alpha=c["alpha"], tau=c["tau"], l_0=c["l_0"],
                  optim_config={"name": "adam", "lr": c["lr"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"], epsilon_min=c["epsilon_min"],
                  explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"], start_train_step=c["start"], target_update_period=c["target"],
                  lr_decay=c["lr_decay"], run_step=c["run_step"], device="cpu")
    return refkit.value_cartpole_curve(agent, seed, c["steps"], c["chunk"])


def gen_curves(out_dir, threads):
    curves = refkit.seeded_curves(reference_curve, CURVE_SEEDS, "mdqn")
    doc = refkit.curve_doc("tools/gen_golden_mdqn.py --only curves (the unmodified reference M_DQN, CPU, scratch copy)", CURVE_SEEDS, threads,
                           mdqn_cartpole={"config": CURVE_CONFIG, "metric": "mean episode length per 1000 env steps", "reference": curves})
    refkit.write_curves(os.path.join(out_dir, "curves_reference_mdqn.json"), doc)


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS), gen_curves, threads=8)
