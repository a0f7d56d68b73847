#!/usr/bin/env python3
"""Golden vectors of Munchausen IQN, from the UNMODIFIED reference agent (core/agent/m_iqn.py on core/network/iqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  The reference is staged exactly as oracle/gen_golden.py stages it (scratch copy, no bytecode, one torch thread)
and `M_IQN.learn()` runs under gen_golden's line tap; this file holds none of the reference's code.  The FOUR tau draws of a learn()
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
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import synth  # noqa: E402
from oracle.gen_golden import RECIPE_SEED, LineTap, _fill, flat, sd_to_np  # noqa: E402
from gen_golden_iqn import MAX_BYTES, SPECS as IQN_SPECS, THIN_STRIDE, thin  # noqa: E402

M_HYPER = dict(alpha=0.9, tau=0.03, l_0=-1)
SPECS = {"m" + k: v for k, v in IQN_SPECS.items()}
# locals in front of optimizer.zero_grad; `logit` there is the FOURTH forward's output (stored as logit_again)
TAPPED = ["logit", "logit_target", "target_q", "next_target_q", "theta_pred", "theta_target", "log_policy", "clipped_log_policy", "munchausen_term",
          "maximum_entropy_term", "loss", "state", "action", "reward", "next_state", "done"]


def gen_fixture(name, out_dir):
    import torch
    from core.agent.m_iqn import M_IQN
    from core.network.iqn import IQN as IQNNet

    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu")
    kw.update(SPECS[name])
    kw.update(M_HYPER)
    S, A, E, N, B = kw["state_size"], kw["action_size"], kw["embedding_dim"], kw["num_sample"], kw["batch_size"]
    torch.manual_seed(3)
    np.random.seed(3)
    agent = M_IQN(**kw)
    shapes = {k: tuple(v.shape) for k, v in agent.network.state_dict().items()}
    H = shapes["l1.weight"][0]
    with torch.no_grad():
        for net, seed in ((agent.network, RECIPE_SEED), (agent.target_network, RECIPE_SEED + 1)):
            rec = synth.recipe_state_dict(shapes, seed)
            for k, p in net.named_parameters():
                p.copy_(torch.from_numpy(rec[k]))
    agent.memory.first_store = False
    _fill(agent, 200, S, A, np.random.RandomState(17))
    sd0, sdt = sd_to_np(agent.network.state_dict()), sd_to_np(agent.target_network.state_dict())
    out = {}
    n = agent.memory.size
    for k in agent.memory.buffer[0].keys():
        out[f"buf_{k}"] = np.concatenate([agent.memory.buffer[i][k] for i in range(n)], 0)

    taus = []
    inner = IQNNet.make_embed

    def recording(self, x, tau_min, tau_max):
        res = inner(self, x, tau_min, tau_max)
        taus.append(res[1].detach().numpy().copy())
        return res

    tap = LineTap(M_IQN.learn, {"first": ("action_eye = torch.eye", []), "pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])})
    graw, head, first = {}, {}, []

    def on_first(frame):
        t = frame.f_locals["logit"]  # the first forward's output, with its graph
        t.retain_grad()
        first.append(t)
        head["logit"] = t.detach().numpy().copy()

    def on_step(frame):
        graw.update({k: p.grad.detach().numpy().copy() for k, p in agent.network.named_parameters()})
        head["d_logit"] = first[0].grad.detach().numpy().copy()

    tap.on_line["first"], tap.on_line["step"] = on_first, on_step
    np.random.seed(42)
    torch.manual_seed(42)
    IQNNet.make_embed = recording
    try:
        with tap:
            result = agent.learn()
    finally:
        IQNNet.make_embed = inner
    assert len(first) == 1 and len(taus) == 4 and all(t.shape == (B, N, 1) for t in taus)
    out["learn/tau"] = np.stack([t.reshape(B, N) for t in taus])  # [4][B][N]: online(s), online(s'), target(s'), online(s) again
    rec = dict(tap.records["pre_step"][0])
    rec["logit_again"] = rec.pop("logit")
    flat("learn/", rec, out)
    flat("learn/", head, out)
    assert out["learn/logit"].shape == (B, N, A) and out["learn/d_logit"].shape == (B, N, A) and out["learn/logit_again"].shape == (B, N, A)
    assert not np.array_equal(out["learn/logit"], out["learn/logit_again"]) and out["learn/theta_target"].shape == (B, N, 1)
    sd1 = sd_to_np(agent.network.state_dict())
    out["fill"], out["fill_seed"], out["recipe_seed"], out["thin_stride"] = np.asarray(200), np.asarray(17), np.asarray(RECIPE_SEED), np.asarray(THIN_STRIDE)
    flat("grad_thin/", {k: thin(v) for k, v in graw.items()}, out)
    out["grad_norm"] = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in graw.values()))
    for k, v in graw.items():
        out[f"grad_absmax/{k}"] = np.abs(v).max()
    # the initial weights come back from the recipe: only the three biggest tensors' samples are stored, to pin the regeneration
    flat("sd0_thin/", {k: thin(v) for k, v in sd0.items() if v.size > 8192}, out)
    flat("sdt_thin/", {k: thin(v) for k, v in sdt.items() if v.size > 8192}, out)
    flat("sd1_thin/", {k: thin(v) for k, v in sd1.items()}, out)
    for st_key in ("exp_avg", "exp_avg_sq"):
        for k, p in agent.network.named_parameters():
            out[f"opt1_thin/{st_key}/{k}"] = thin(agent.optimizer.state[p][st_key].detach().numpy())
    for k, v in shapes.items():
        out[f"shape/{k}"] = np.asarray(v, dtype=np.int64)
    for k, v in result.items():
        out[f"result/{k}"] = np.asarray(v)
    hyper = dict(gamma=0.99, lr=kw["optim_config"]["lr"], B=B, S=S, A=A, H=H, E=E, N=N, sample_min=0.0, sample_max=1.0, alpha=M_HYPER["alpha"], m_tau=M_HYPER["tau"],
                 l_0=M_HYPER["l_0"], np_seed=42, torch_seed=42)
    hyper.update({f"optim_{k}": v for k, v in kw["optim_config"].items() if isinstance(v, (int, float, bool))})
    for k, v in hyper.items():
        out[f"hyper/{k}"] = np.asarray(v)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    lp = out["learn/log_policy"]
    print(name, {k: float(v) for k, v in result.items()}, f"{size} bytes; rows with a clipped log-policy: {int((lp < M_HYPER['l_0']).sum())} of {B}")
    assert size <= MAX_BYTES, f"{name}.npz: {size} bytes, more than the family's largest fixture ({MAX_BYTES})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (the directory that holds jorldy/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    out_dir = os.path.abspath(args.out)
    os.makedirs(out_dir, exist_ok=True)
    scratch = tempfile.mkdtemp(prefix="jref_")
    subprocess.check_call(f"cd {args.ref} && tar --exclude='jorldy/core/env/mlagents' -cf - jorldy | (cd {scratch} && tar xf -)", shell=True)
    cwd = os.getcwd()
    os.chdir(os.path.join(scratch, "jorldy"))
    sys.path.insert(0, os.getcwd())
    sys.dont_write_bytecode = True
    import torch

    try:
        torch.set_num_threads(1)  # deterministic reductions in the fixtures
        for name in SPECS:
            gen_fixture(name, out_dir)
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    print("written to", out_dir)


if __name__ == "__main__":
    main()
