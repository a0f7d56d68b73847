#!/usr/bin/env python3
"""Golden vectors of Munchausen IQN, from the UNMODIFIED reference agent (core/agent/m_iqn.py on core/network/iqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  Staging, the main, the line tap under which `M_IQN.learn()` runs and the value family's recorder are oracle/refkit.py's;
what IQN's fixtures share with these is tools/gen_golden_iqn.py's; this file holds none of the reference's code.  The FOUR tau draws of a learn()
(online(s), online(s'), target(s'), online(s) again, in that order: m_iqn.py:30, 40, 43, 50) are recorded by wrapping the network
class's make_embed at run time.  `logit` names two tensors in that learn(): the first forward's output is taken (and its gradient
retained) in front of line 32, the fourth forward's -- which line 50 assigns to the same name -- in front of optimizer.zero_grad.

The specs are tools/gen_golden_iqn.py's plus the config's alpha, tau, l_0; the weights come from synth.recipe_state_dict (seed and
seed + 1 for online and target) and the big tensors are stored thinned with the same stride.

  tests/golden/miqn.npz            S 4, A 3, E 16, N 8, B 32, Adam 1e-3
  tests/golden/miqn_odd.npz        S 4, A 5, E 10, N 33, B 7
  tests/golden/miqn_cartpole.npz   config.m_iqn.cartpole exactly (A 2, E 64, N 64, B 32, Adam 1e-4, eps 1e-2 / 32, alpha 0.9, tau 0.03, l_0 -1)

No learning curve: the M-DQN and IQN curves cover both halves, and a reference M-IQN curve costs over an hour of CPU.

Usage:  python tools/gen_golden_miqn.py --ref <reference checkout> [--out tests/golden]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import refkit  # noqa: E402
from gen_golden_iqn import SPECS as IQN_SPECS, agent_kwargs, finish, recording_taus, tau_entry  # noqa: E402

M_HYPER = dict(alpha=0.9, tau=0.03, l_0=-1)
SPECS = {"m" + k: v for k, v in IQN_SPECS.items()}
# locals in front of optimizer.zero_grad; `logit` there is the FOURTH forward's output (stored as logit_again)
TAPPED = ["logit", "logit_target", "target_q", "next_target_q", "theta_pred", "theta_target", "log_policy", "clipped_log_policy", "munchausen_term",
          "maximum_entropy_term", "loss", "state", "action", "reward", "next_state", "done"]


MARKERS = {"first": ("action_eye = torch.eye", []), "pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])}


def gen_fixture(name, out_dir):
    from core.agent.m_iqn import M_IQN

    kw = agent_kwargs(SPECS[name])
    kw.update(M_HYPER)
    agent, out = refkit.value_agent(M_IQN, kw, recipe=True)
    taus = []
    # the first forward's output, with its graph, is the local `logit` in front of the marker "first"
    step, result = refkit.record_value_learn(agent, MARKERS, out, watch="logit", at="first", name="logit", rename={"logit": "logit_again"}, around=recording_taus(taus),
                                             first=lambda: tau_entry(taus, kw))
    assert len(taus) == 4  # online(s), online(s'), target(s'), online(s) again
    B, N, A = kw["batch_size"], kw["num_sample"], kw["action_size"]
    assert out["learn/logit_again"].shape == (B, N, A) and not np.array_equal(out["learn/logit"], out["learn/logit_again"]) and out["learn/theta_target"].shape == (B, N, 1)
    clipped = int((out["learn/log_policy"] < M_HYPER["l_0"]).sum())
    finish(out_dir, name, out, agent, kw, step, result, note=f"rows with a clipped log-policy: {clipped} of {B}", alpha=M_HYPER["alpha"], m_tau=M_HYPER["tau"], l_0=M_HYPER["l_0"])


if __name__ == "__main__":
    refkit.run(refkit.each(gen_fixture, SPECS))
