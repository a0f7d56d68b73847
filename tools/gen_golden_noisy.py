#!/usr/bin/env python3
"""Golden vectors of the NoisyNet agent, from the UNMODIFIED reference agent (core/agent/noisy.py on core/network/noisy.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `Noisy.learn()` runs on the CPU and the value family's recorder are oracle/refkit.py's;
this file holds none of the reference's code.

  tests/golden/noisy.npz       S 4, A 3, H 32, B 32, factorised noise, Adam 1e-3, perturbed online and target weights: every tensor stored
  tests/golden/noisy_odd.npz   S 4, A 5, H 64, B 7, independent noise
  tests/golden/noisy_cnn.npz   uint8 frames (4, 44, 52), A 6, H 32, B 8, factorised noise: F = 64 * 2 * 3 features of a non-square map;
                               recipe weights (regenerated from the seed by the test), large tensors thinned (oracle/synth.py)

The NoisyNet draws happen inside the reference's forward (utils.py:58-60, 75-76) on torch's CPU generator: each fixture stores the seed
set immediately in front of learn() (hyper/torch_seed), from which a test regenerates them in order -- network(state): layer 1 (input
side, output side), layer 2; then target_network(next_state) likewise.

Usage:  python tools/gen_golden_noisy.py --ref <reference checkout> [--out tests/golden]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refkit, synth  # noqa: E402
from oracle.refkit import FILL_SEED, RECIPE_SEED  # noqa: E402

SPECS = {
    "noisy": dict(state_size=4, action_size=3, hidden_size=32, batch_size=32, noise_type="factorized", head="mlp", fill=200, recipe=False),
    "noisy_odd": dict(state_size=4, action_size=5, hidden_size=64, batch_size=7, noise_type="independent", head="mlp", fill=200, recipe=False),
    "noisy_cnn": dict(state_size=(4, 44, 52), action_size=6, hidden_size=32, batch_size=8, noise_type="factorized", head="cnn", fill=24, recipe=True),
}
# locals of Noisy.learn in front of optimizer.zero_grad: `q` there is the TAKEN q [B, 1]; network(state, True) itself is kept by the recorder's forward hook (q_all)
TAPPED = ["q", "next_q", "target_q", "loss", "action", "reward", "done"]
TAPPED_VECTORS = ["state", "next_state"]  # stored for vector observations only (frames: the replay columns hold them already)
LR = 1e-3


def gen_fixture(name, out_dir):
    from core.agent.noisy import Noisy

    spec = dict(SPECS[name])
    recipe, n_fill = spec.pop("recipe"), spec.pop("fill")
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu", network="noisy",
              optim_config={"name": "adam", "lr": LR})
    kw.update(spec)
    agent, out = refkit.value_agent(Noisy, kw, recipe, fill=n_fill)
    markers = {"pre_step": ("self.optimizer.zero_grad", TAPPED + ([] if kw["head"] == "cnn" else TAPPED_VECTORS)), "step": ("self.optimizer.step()", [])}
    step, result = refkit.record_value_learn(agent, markers, out)
    assert out["learn/q_all"].shape == (kw["batch_size"], kw["action_size"])
    if recipe:
        out["recipe_seed"] = np.asarray(RECIPE_SEED)
    refkit.store_step(out, agent, *step, thin=synth.thin if recipe else None, moments=("exp_avg", "exp_avg_sq"), norm=False)
    refkit.put_result(out, result)
    refkit.put_hyper(out, dict(gamma=0.99, lr=LR, B=kw["batch_size"], A=kw["action_size"], H=kw["hidden_size"], np_seed=42, torch_seed=42, fill=n_fill, fill_seed=FILL_SEED,
                               S=kw["state_size"], noise_type=kw["noise_type"], head=kw["head"]))
    refkit.save_fixture(out_dir, name, out, cap=1 << 20)  # what a committed file may have


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS))
