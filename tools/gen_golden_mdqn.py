#!/usr/bin/env python3
"""Golden vectors and the reference learning curve of Munchausen DQN, from the UNMODIFIED reference agent (core/agent/m_dqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  The reference is staged exactly as oracle/gen_golden.py stages it (scratch copy, no bytecode, one torch thread
for the fixtures) and `M_DQN.learn()` runs under gen_golden's line tap; this file holds none of the reference's code.

  tests/golden/mdqn.npz            S 4, A 3, H 32, B 32, discrete_q_network, Adam 1e-3, perturbed online and target weights: every tensor stored
  tests/golden/mdqn_odd.npz        S 4, A 5, H 64, B 7, network "dueling"
  tests/golden/mdqn_cartpole.npz   config.m_dqn.cartpole exactly (H 512, B 32, Adam 1e-4, alpha 0.9, tau 0.03, l_0 -1): recipe weights, thinned
  tests/golden/curves_reference_mdqn.json   config.m_dqn.cartpole in the single-mode loop of tests/test_learning_curve_gpu.py::_dqn_curve

Usage:  python tools/gen_golden_mdqn.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 8]
"""
import argparse
import json
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

M_HYPER = dict(alpha=0.9, tau=0.03, l_0=-1)
SPECS = {
    "mdqn": dict(state_size=4, action_size=3, hidden_size=32, batch_size=32, network="discrete_q_network", optim_config={"name": "adam", "lr": 1e-3}, recipe=False),
    "mdqn_odd": dict(state_size=4, action_size=5, hidden_size=64, batch_size=7, network="dueling", optim_config={"name": "adam", "lr": 1e-3}, recipe=False),
    "mdqn_cartpole": dict(state_size=4, action_size=2, hidden_size=512, batch_size=32, network="discrete_q_network", optim_config={"name": "adam", "lr": 1e-4},
                          recipe=True),
}
# locals of M_DQN.learn in front of optimizer.zero_grad: `q` there is the TAKEN q [B, 1]; network(state) itself is rebuilt below (q_all)
TAPPED = ["q", "next_target_q", "target_q", "clipped_log_policy", "munchausen_term", "maximum_entropy_term", "loss", "state", "action", "reward", "next_state", "done"]

CURVE_STEPS, CURVE_RUN_STEP, CURVE_CHUNK, CURVE_SEEDS = 12000, 15000, 1000, (1, 2, 3)
CURVE_CONFIG = dict(steps=CURVE_STEPS, chunk=CURVE_CHUNK, run_step=CURVE_RUN_STEP, hidden=512, batch=32, alpha=0.9, tau=0.03, l_0=-1, lr=1e-4, gamma=0.99,
                    epsilon_init=1.0, epsilon_min=0.01, explore_ratio=0.2, start=2000, target=500, buffer=50000, lr_decay=True)


def gen_fixture(name, out_dir):
    import torch
    from core.agent.m_dqn import M_DQN

    spec = dict(SPECS[name])
    recipe = spec.pop("recipe")
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu")
    kw.update(spec)
    kw.update(M_HYPER)
    S, A, H, B = kw["state_size"], kw["action_size"], kw["hidden_size"], kw["batch_size"]
    torch.manual_seed(3)
    np.random.seed(3)
    agent = M_DQN(**kw)
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
    _fill(agent, 200, S, A, np.random.RandomState(17))
    sd0, sdt = sd_to_np(agent.network.state_dict()), sd_to_np(agent.target_network.state_dict())
    out = {}
    n = agent.memory.size
    for k in agent.memory.buffer[0].keys():
        out[f"buf_{k}"] = np.concatenate([agent.memory.buffer[i][k] for i in range(n)], 0)

    tap = LineTap(M_DQN.learn, {"pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])})
    graw, head = {}, {}
    # network(state) is an unnamed temporary inside learn(): a forward hook keeps the tensor itself, so that its .grad is d loss / d network(state)
    seen = []
    hook = agent.network.register_forward_hook(lambda mod, inp, outp: seen.append(outp))

    def on_pre(frame):
        seen[-1].retain_grad()
        head["q_all"] = seen[-1].detach().numpy().copy()
        with torch.no_grad():
            head["target_q_state"] = agent.target_network(frame.f_locals["state"]).detach().numpy().copy()

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
    if recipe:
        out["fill"], out["fill_seed"], out["recipe_seed"] = np.asarray(200), np.asarray(17), np.asarray(RECIPE_SEED)
        flat("grad_thin/", {k: synth.thin(v) for k, v in graw.items()}, out)
        out["grad_norm"] = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in graw.values()))
        for k, v in graw.items():
            out[f"grad_absmax/{k}"] = np.abs(v).max()
        flat("sd0_thin/", {k: synth.thin(v) for k, v in sd0.items()}, out)
        flat("sdt_thin/", {k: synth.thin(v) for k, v in sdt.items()}, out)
        flat("sd1_thin/", {k: synth.thin(v) for k, v in sd1.items()}, out)
        for st_key in ("exp_avg", "exp_avg_sq"):
            for k, p in agent.network.named_parameters():
                out[f"opt1_thin/{st_key}/{k}"] = synth.thin(agent.optimizer.state[p][st_key].detach().numpy())
    else:
        flat("grad/", graw, out)
        flat("sd0/", sd0, out)
        flat("sdt/", sdt, out)
        flat("sd1/", sd1, out)
    for k, v in result.items():
        out[f"result/{k}"] = np.asarray(v)
    hyper = dict(gamma=0.99, lr=kw["optim_config"]["lr"], B=B, S=S, A=A, H=H, alpha=M_HYPER["alpha"], m_tau=M_HYPER["tau"], l_0=M_HYPER["l_0"], np_seed=42, torch_seed=42)
    hyper.update({f"optim_{k}": v for k, v in kw["optim_config"].items() if isinstance(v, (int, float, bool))})
    for k, v in hyper.items():
        out[f"hyper/{k}"] = np.asarray(v)
    out["hyper/network"] = np.asarray(kw["network"])
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(name, {k: float(v) for k, v in result.items()}, f"{os.path.getsize(path)} bytes")


def reference_curve(seed):
    """The loop of tests/test_learning_curve_gpu.py::_dqn_curve with the reference's M_DQN on the oracle's CartPole."""
    import torch
    from core.agent.m_dqn import M_DQN

    from oracle.dqn_port import make_env

    c = CURVE_CONFIG
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = M_DQN(state_size=4, action_size=2, hidden_size=c["hidden"], network="discrete_q_network", alpha=c["alpha"], tau=c["tau"], l_0=c["l_0"],
                  optim_config={"name": "adam", "lr": c["lr"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"], epsilon_min=c["epsilon_min"],
                  explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"], start_train_step=c["start"], target_update_period=c["target"],
                  lr_decay=c["lr_decay"], run_step=c["run_step"], device="cpu")
    env, state = make_env(1000 + seed)
    out, lens, ep = [], [], 0
    for step in range(1, c["steps"] + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"]).reshape(-1))
        tr = {"state": state, "next_state": nxt.astype(np.float32), "reward": rew.reshape(1, 1).astype(np.float64), "done": done.reshape(1, 1)}
        tr.update(a)
        agent.process([tr], step)
        state = env.obs().astype(np.float32)
        ep += 1
        if bool(done.reshape(-1)[0]):
            lens.append(ep)
            ep = 0
        if step % c["chunk"] == 0:
            out.append(float(np.mean(lens)) if lens else float(ep))
            lens = []
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (the directory that holds jorldy/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default="fixtures,curves")
    ap.add_argument("--threads", type=int, default=8, help="torch threads of the curve runs (the fixtures always use one)")
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
        todo = args.only.split(",")
        if "fixtures" in todo:
            torch.set_num_threads(1)  # deterministic reductions in the fixtures
            for name in SPECS:
                gen_fixture(name, out_dir)
        if "curves" in todo:
            torch.set_num_threads(args.threads)
            curves = []
            for s in CURVE_SEEDS:
                curves.append(reference_curve(s))
                print("curve seed", s, [round(v, 1) for v in curves[-1]], flush=True)
            doc = {"generator": "tools/gen_golden_mdqn.py --only curves (the unmodified reference M_DQN, CPU, scratch copy)", "seeds": list(CURVE_SEEDS),
                   "torch_threads": args.threads,
                   "mdqn_cartpole": {"config": CURVE_CONFIG, "metric": "mean episode length per 1000 env steps", "reference": curves}}
            with open(os.path.join(out_dir, "curves_reference_mdqn.json"), "w") as f:
                json.dump(doc, f, indent=1)
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    print("written to", out_dir)


if __name__ == "__main__":
    main()
