#!/usr/bin/env python3
"""Golden vectors of the NoisyNet agent, from the UNMODIFIED reference agent (core/agent/noisy.py on core/network/noisy.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  The reference is staged exactly as oracle/gen_golden.py stages it (scratch copy, no bytecode, one torch thread)
and `Noisy.learn()` runs on the CPU under gen_golden's line tap; this file holds none of the reference's code.

  tests/golden/noisy.npz       S 4, A 3, H 32, B 32, factorised noise, Adam 1e-3, perturbed online and target weights: every tensor stored
  tests/golden/noisy_odd.npz   S 4, A 5, H 64, B 7, independent noise
  tests/golden/noisy_cnn.npz   uint8 frames (4, 44, 52), A 6, H 32, B 8, factorised noise: F = 64 * 2 * 3 features of a non-square map;
                               recipe weights (regenerated from the seed by the test), large tensors thinned (oracle/synth.py)

The NoisyNet draws happen inside the reference's forward (utils.py:58-60, 75-76) on torch's CPU generator: each fixture stores the seed
set immediately in front of learn() (hyper/torch_seed), from which a test regenerates them in order -- network(state): layer 1 (input
side, output side), layer 2; then target_network(next_state) likewise.

Usage:  python tools/gen_golden_noisy.py --ref <reference checkout> [--out tests/golden]
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
from oracle import synth  # noqa: E402
from oracle.gen_golden import RECIPE_SEED, LineTap, _fill, flat, sd_to_np  # noqa: E402

SPECS = {
    "noisy": dict(state_size=4, action_size=3, hidden_size=32, batch_size=32, noise_type="factorized", head="mlp", fill=200, recipe=False),
    "noisy_odd": dict(state_size=4, action_size=5, hidden_size=64, batch_size=7, noise_type="independent", head="mlp", fill=200, recipe=False),
    "noisy_cnn": dict(state_size=(4, 44, 52), action_size=6, hidden_size=32, batch_size=8, noise_type="factorized", head="cnn", fill=24, recipe=True),
}
# locals of Noisy.learn in front of optimizer.zero_grad: `q` there is the TAKEN q [B, 1]; network(state, True) itself is kept by a hook (q_all)
TAPPED = ["q", "next_q", "target_q", "loss", "action", "reward", "done"]
TAPPED_VECTORS = ["state", "next_state"]  # stored for vector observations only (frames: the replay columns hold them already)
LR = 1e-3


def gen_fixture(name, out_dir):
    import torch
    from core.agent.noisy import Noisy

    spec = dict(SPECS[name])
    recipe, n_fill = spec.pop("recipe"), spec.pop("fill")
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu", network="noisy",
              optim_config={"name": "adam", "lr": LR})
    kw.update(spec)
    S, A, H, B = kw["state_size"], kw["action_size"], kw["hidden_size"], kw["batch_size"]
    cnn = kw["head"] == "cnn"
    torch.manual_seed(3)
    np.random.seed(3)
    agent = Noisy(**kw)
    with torch.no_grad():
        if recipe:
            shapes = {k: v.shape for k, v in agent.network.state_dict().items()}
            for net, seed in ((agent.network, RECIPE_SEED), (agent.target_network, RECIPE_SEED + 1)):
                rec = synth.recipe_state_dict(shapes, seed)
                for k, p in net.named_parameters():
                    p.copy_(torch.from_numpy(rec[k]))
        else:
            for net in (agent.network, agent.target_network):  # independent draws: the target differs from the online net
                for p in net.parameters():
                    p.add_(0.1 * torch.randn_like(p))
    agent.memory.first_store = False
    _fill(agent, n_fill, S, A, np.random.RandomState(17))
    sd0, sdt = sd_to_np(agent.network.state_dict()), sd_to_np(agent.target_network.state_dict())
    out = {}
    n = agent.memory.size
    for k in agent.memory.buffer[0].keys():
        out[f"buf_{k}"] = np.concatenate([agent.memory.buffer[i][k] for i in range(n)], 0)

    tap = LineTap(Noisy.learn, {"pre_step": ("self.optimizer.zero_grad", TAPPED + ([] if cnn else TAPPED_VECTORS)), "step": ("self.optimizer.step()", [])})
    graw, head = {}, {}
    # network(state, True) is an unnamed temporary inside learn(): a forward hook keeps the tensor itself, so that its .grad is d loss / d network(state)
    seen = []
    hook = agent.network.register_forward_hook(lambda mod, inp, outp: seen.append(outp))

    def on_pre(frame):
        seen[-1].retain_grad()
        head["q_all"] = seen[-1].detach().numpy().copy()

    def on_step(frame):
        graw.update({k: p.grad.detach().numpy().copy() for k, p in agent.network.named_parameters()})
        head["d_q_all"] = seen[-1].grad.detach().numpy().copy()

    tap.on_line["pre_step"], tap.on_line["step"] = on_pre, on_step
    np.random.seed(42)
    torch.manual_seed(42)
    with tap:
        result = agent.learn()
    hook.remove()
    assert len(seen) == 1 and head["q_all"].shape == (B, A)
    flat("learn/", tap.records["pre_step"][0], out)
    flat("learn/", head, out)
    sd1 = sd_to_np(agent.network.state_dict())
    moments = {st_key: {k: agent.optimizer.state[p][st_key].detach().numpy().copy() for k, p in agent.network.named_parameters()} for st_key in ("exp_avg", "exp_avg_sq")}
    if recipe:
        out["recipe_seed"] = np.asarray(RECIPE_SEED)
        flat("grad_thin/", {k: synth.thin(v) for k, v in graw.items()}, out)
        for k, v in graw.items():
            out[f"grad_absmax/{k}"] = np.abs(v).max()
        flat("sd0_thin/", {k: synth.thin(v) for k, v in sd0.items()}, out)
        flat("sdt_thin/", {k: synth.thin(v) for k, v in sdt.items()}, out)
        flat("sd1_thin/", {k: synth.thin(v) for k, v in sd1.items()}, out)
        for st_key, d in moments.items():
            flat(f"opt1_thin/{st_key}/", {k: synth.thin(v) for k, v in d.items()}, out)
    else:
        flat("grad/", graw, out)
        flat("sd0/", sd0, out)
        flat("sdt/", sdt, out)
        flat("sd1/", sd1, out)
        for st_key, d in moments.items():
            flat(f"opt1/{st_key}/", d, out)
    for k, v in result.items():
        out[f"result/{k}"] = np.asarray(v)
    hyper = dict(gamma=0.99, lr=LR, B=B, A=A, H=H, np_seed=42, torch_seed=42, fill=n_fill, fill_seed=17)
    for k, v in hyper.items():
        out[f"hyper/{k}"] = np.asarray(v)
    out["hyper/S"] = np.asarray(S)
    out["hyper/noise_type"], out["hyper/head"] = np.asarray(kw["noise_type"]), np.asarray(kw["head"])
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= (1 << 20), f"{path}: {size} bytes is more than a committed file may have"
    print(name, {k: float(v) for k, v in result.items()}, f"{size} bytes")


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
