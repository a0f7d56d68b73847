#!/usr/bin/env python3
"""Golden vectors and the reference learning curve of IQN, from the UNMODIFIED reference agent (core/agent/iqn.py, core/network/iqn.py).

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or
reads the reference.  The reference is staged exactly as oracle/gen_golden.py stages it (scratch copy, no bytecode, one torch thread
for the fixtures) and `IQN.learn()` runs under gen_golden's line tap; this file holds none of the reference's code.  The three tau
draws of a learn() (online(s), online(s'), target(s'), in that order) are recorded by wrapping the network class's make_embed at run time.

The reference builds its network without hidden_size (agent/iqn.py:44-49), so it is 512 wide in every fixture: the weights come from
synth.recipe_state_dict (seed and seed + 1 for online and target) and the big tensors are stored thinned, as mdqn_cartpole.npz does.

  tests/golden/iqn.npz            S 4, A 3, E 16, N 8, B 32, Adam 1e-3
  tests/golden/iqn_odd.npz        S 4, A 5, E 10, N 33, B 7
  tests/golden/iqn_cartpole.npz   config.iqn.cartpole exactly (A 2, E 64, N 64, B 32, Adam 1e-4, eps 1e-2 / 32)
  tests/golden/curves_reference_iqn.json   config.iqn.cartpole in the single-mode loop of tests/test_learning_curve_gpu.py::_dqn_curve

Usage:  python tools/gen_golden_iqn.py --ref <reference checkout> [--out tests/golden] [--only fixtures|curves] [--threads 8]
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


def gen_fixture(name, out_dir):
    import torch
    from core.agent.iqn import IQN
    from core.network.iqn import IQN as IQNNet

    spec = dict(SPECS[name])
    kw = dict(gamma=0.99, buffer_size=256, start_train_step=0, target_update_period=10000, run_step=100000, device="cpu")
    kw.update(spec)
    S, A, E, N, B = kw["state_size"], kw["action_size"], kw["embedding_dim"], kw["num_sample"], kw["batch_size"]
    torch.manual_seed(3)
    np.random.seed(3)
    agent = IQN(**kw)
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

    tap = LineTap(IQN.learn, {"pre_step": ("self.optimizer.zero_grad", TAPPED), "step": ("self.optimizer.step()", [])})
    graw, head = {}, {}

    def on_pre(frame):
        frame.f_locals["logit"].retain_grad()

    def on_step(frame):
        graw.update({k: p.grad.detach().numpy().copy() for k, p in agent.network.named_parameters()})
        head["d_logit"] = frame.f_locals["logit"].grad.detach().numpy().copy()

    tap.on_line["pre_step"], tap.on_line["step"] = on_pre, on_step
    np.random.seed(42)
    torch.manual_seed(42)
    IQNNet.make_embed = recording
    try:
        with tap:
            result = agent.learn()
    finally:
        IQNNet.make_embed = inner
    assert len(taus) == 3 and all(t.shape == (B, N, 1) for t in taus)
    out["learn/tau"] = np.stack([t.reshape(B, N) for t in taus])  # [3][B][N]: online(s), online(s'), target(s')
    flat("learn/", tap.records["pre_step"][0], out)
    flat("learn/", head, out)
    assert out["learn/logit"].shape == (B, N, A) and out["learn/d_logit"].shape == (B, N, A)
    gap, bound = near_tie_bound(out["learn/logit_next"])
    assert (gap > bound).all(), f"{name}: a row with a near-tie of the two best next actions (gap {gap.min():.3e}); pick another fill seed"
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
    hyper = dict(gamma=0.99, lr=kw["optim_config"]["lr"], B=B, S=S, A=A, H=H, E=E, N=N, sample_min=0.0, sample_max=1.0, np_seed=42, torch_seed=42)
    hyper.update({f"optim_{k}": v for k, v in kw["optim_config"].items() if isinstance(v, (int, float, bool))})
    for k, v in hyper.items():
        out[f"hyper/{k}"] = np.asarray(v)
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(name, {k: float(v) for k, v in result.items()}, f"{size} bytes")
    assert size <= MAX_BYTES, f"{name}.npz: {size} bytes, more than the family's largest fixture ({MAX_BYTES})"


def reference_curve(seed):
    """The loop of tests/test_learning_curve_gpu.py::_dqn_curve with the reference's IQN on the oracle's CartPole."""
    import torch
    from core.agent.iqn import IQN

    from oracle.dqn_port import make_env

    c = CURVE_CONFIG
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = IQN(state_size=4, action_size=2, network="iqn", num_sample=c["num_sample"], embedding_dim=c["embedding_dim"], sample_min=c["sample_min"],
                sample_max=c["sample_max"], optim_config={"name": "adam", "lr": c["lr"], "eps": c["eps"]}, gamma=c["gamma"], epsilon_init=c["epsilon_init"],
                epsilon_min=c["epsilon_min"], explore_ratio=c["explore_ratio"], buffer_size=c["buffer"], batch_size=c["batch"], start_train_step=c["start"],
                target_update_period=c["target"], lr_decay=c["lr_decay"], run_step=c["run_step"], device="cpu")
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


def curve_learns(curves):
    """The reference's side of the DQN curve test's criteria (tests/test_learning_curve_gpu.py): starts near random play, and learns."""
    start, end = np.mean([np.mean(x[:2]) for x in curves]), np.mean([np.mean(x[-4:]) for x in curves])
    return bool(start < 40 and end > 4 * start), float(start), float(end)


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
            ok, start, end = curve_learns(curves)
            print(f"reference IQN episode length {start:.1f} -> {end:.1f}: {'learns' if ok else 'DOES NOT LEARN'} by the DQN curve test's criteria", flush=True)
            doc = {"generator": "tools/gen_golden_iqn.py --only curves (the unmodified reference IQN, CPU, scratch copy)", "seeds": list(CURVE_SEEDS),
                   "torch_threads": args.threads, "reference_learns": ok,
                   "iqn_cartpole": {"config": CURVE_CONFIG, "metric": "mean episode length per 1000 env steps", "reference": curves}}
            with open(os.path.join(out_dir, "curves_reference_iqn.json"), "w") as f:
                json.dump(doc, f, indent=1)
            assert ok, "the reference curve does not show learning within these steps: say in DESIGN.md which assertions the curve test keeps"
    finally:
        os.chdir(cwd)
        shutil.rmtree(scratch, ignore_errors=True)
    print("written to", out_dir)


if __name__ == "__main__":
    main()
