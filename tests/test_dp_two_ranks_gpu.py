"""The native data-parallel learners with TWO ranks (VERDICT r2 "missing" #1): two processes on cuda:0,
process group gloo (RCCL refuses two ranks on one device), native PPO at config.ppo.cartpole widths and native Rainbow at
B = 32, each rank with its own rollout / replay shard and its own index lists.

  (a) after the updates the ranks' parameter buckets are bit-identical;
  (b) PPO == ONE learner on the concatenated batch fed the same per-rank index lists (the reference shuffles globally,
      core/agent/ppo.py:116-120; here: 16 workers x 128 steps, minibatch 512 = [rank 0's 256 rows; rank 1's 256 rows]) at the config's
      own learning rate, i.e. with the value clamp active: the critic's max(mean, mean) is taken over the global minibatch;
  (c) the sharded PER importance weights == those of a single logical sum tree over both shards (per_buffer.py:88-94);
  (d) `bench.py --gpus 2` runs 3 steps through the same launch / pinning / barrier plumbing.
The same checks with rank r on GPU r over RCCL live in tests/test_zz_rccl_two_gpus_gpu.py (they need two GPUs, and run last).
"""
import os
import socket
import subprocess
import sys

import numpy as np

import margins
import pytest
import torch

from tests import dp_worker as W
from tests.util import npy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_ranks(mode, tmp_path, world=2, backend="gloo", extra_env=None):
    port = _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", JH_NO_PIN="1", **(extra_env or {}))
    outs = [str(tmp_path / f"{mode}_{backend}_{r}.npz") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker.py"), mode, str(r), str(world), str(port), outs[r], backend], env=env, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    return [np.load(o) for o in outs]


def test_ppo_native_two_ranks_equal_one_learner_on_the_concatenated_batch(tmp_path, monkeypatch):
    _check_ppo_two_ranks(_run_ranks("ppo", tmp_path), monkeypatch)


PEER = {"JH_DP_COLLECTIVE": "peer"}


def test_peer_pointer_collectives_two_processes_one_gpu(tmp_path):
    """jh_peer_* (round 6, VERDICT r5 #2b): two processes on cuda:0 map each other's arenas through hipIpc handles; the mean of buckets of
    awkward lengths (266 755 = the PPO bucket, 17, 33, ...), many calls in a row, eager and replayed from a hipGraph, and the <= 16-float
    exchange: the exact rank-order fp32 sum on BOTH ranks, no bounded wait gave up."""
    r0, r1 = _run_ranks("peer_unit", tmp_path, extra_env=PEER)
    for r in (r0, r1):
        assert int(r["timeouts"]) == 0 and int(r["done"]) >= 21
        assert float(r["means"].max()) == 0.0, r["means"]       # the same additions in the same order: bit-exact
        assert float(r["smalls"].max()) <= 1e-6, r["smalls"]
        assert float(r["graph_err"].max()) == 0.0, r["graph_err"]
    print(f"peer all-reduce of 266 755 floats, two ranks on one GPU: {float(r0['us_per_allreduce']):.1f} us per call; 2-float exchange: {float(r0['us_per_small']):.1f} us")


def test_ppo_native_two_ranks_through_peer_pointers(tmp_path, monkeypatch):
    """The same equality with one learner on the concatenated batch when the critic sums and the gradient bucket travel through peer
    pointers (no host staging, no collective library)."""
    ranks = _run_ranks("ppo", tmp_path, extra_env=PEER)
    for r in ranks:
        assert int(r["peer_timeouts"]) == 0  # (one process() call: eager; replay from a captured graph is the unit test above)
    _check_ppo_two_ranks(ranks, monkeypatch)


@pytest.mark.parametrize("inject,kind", [("", "rccl"), ("id", "torch"), ("create", "torch")])
def test_rccl_communicator_fallback_is_decided_collectively(inject, kind, monkeypatch):
    """jorldy_amd.parallel.Transport on a 1-rank RCCL group: the library's communicator when everything works; when rank 0 cannot make a
    unique id (a ZERO id is broadcast: every rank still runs the same collectives) or jh_comm_create fails, the all-reduced success flag
    puts ALL ranks on torch.distributed's collectives (a per-rank try/except left ranks on different transports)."""
    import torch.distributed as dist

    from jorldy_amd.parallel import Transport

    if inject:
        monkeypatch.setenv("JH_COMM_INJECT", inject)
    else:
        monkeypatch.delenv("JH_COMM_INJECT", raising=False)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        tr = Transport(dist, None, torch.device("cuda", 0))
        assert tr.kind == kind and tr.capturable
        t = torch.arange(8, dtype=torch.float32, device="cuda")
        tr.mean_(t)
        torch.cuda.synchronize()
        assert torch.equal(t.cpu(), torch.arange(8, dtype=torch.float32))
    finally:
        dist.destroy_process_group()


def _check_ppo_two_ranks(ranks, monkeypatch):
    r0, r1 = ranks
    # (a) identical weights on both ranks, bit for bit
    assert np.array_equal(r0["params"], r1["params"]), "ranks diverged"
    assert np.array_equal(r0["grads"], r1["grads"])
    c = W.PPO_CFG
    M, B, E = c["W"] * c["T"], c["B"], c["E"]
    n_upd = int(r0["n_upd"])
    # (b) one learner: 16 workers (rank 0's rows, then rank 1's), minibatch 512 = the two ranks' minibatches side by side
    agent = W.ppo_agent(2 * c["W"], 2 * B, use_graph=False)
    rows = [W.ppo_rows(0), W.ppo_rows(1)]
    cols = {k: np.concatenate([rows[0][k], rows[1][k]], 0) for k in rows[0]}
    perms = []
    for e in range(E):
        p0, p1 = r0["perms"][e], r1["perms"][e]
        perms.append(np.concatenate([np.concatenate([p0[o:o + B], M + p1[o:o + B]]) for o in range(0, M, B)]))
    from jorldy_amd import np_rng

    def fixed_lists(M_, E_, out):  # stands in for the np.random draws of ppo.py:116-118: the two ranks' lists side by side
        out.reshape(-1)[:] = np.concatenate(perms)
        return out

    agent._predraw = None
    monkeypatch.setattr(np_rng, "epoch_shuffles", fixed_lists)
    agent.process(cols, c["T"])
    monkeypatch.undo()
    torch.cuda.synchronize()
    one = npy(agent._net.params)
    s1 = np.asarray(agent._static["stats_pin"].np[: n_upd + 1], dtype=np.float64)
    s_dp = 0.5 * (r0["stats"].astype(np.float64) + r1["stats"].astype(np.float64))
    # every update's loss terms: mean over 512 rows == mean of the two ranks' means (actor, entropy: exactly linear); the critic is
    # max(mean(e1), mean(e2)) over the GLOBAL minibatch (ppo.py:147-154): both ranks report it (exact DP critic) and it must be
    # the single learner's -- with the value clamp ACTIVE (config's own lr: the branches differ from the third update on)
    for st_ in (r0["stats"], r1["stats"]):
        np.testing.assert_array_equal(st_[:n_upd, 6:8], r0["stats"][:n_upd, 6:8])  # the same global c1 / c2 on every rank, bit for bit
    gap = np.abs(s1[:n_upd, 6] - s1[:n_upd, 7]) / np.maximum(s1[:n_upd, 6], 1e-12)
    assert (gap > 1e-3).sum() >= n_upd // 2, f"the value clamp never became active (relative |c1 - c2| per update: {gap}): the test would not see a wrong branch"
    for j in (6, 7):
        np.testing.assert_allclose(s1[:n_upd, j], r0["stats"][:n_upd, j], rtol=2e-5, atol=1e-7, err_msg="global c1 / c2 vs one learner")
    for j, name in ((1, "actor_loss"), (2, "critic_loss"), (3, "entropy_loss")):
        np.testing.assert_allclose(s1[:n_upd, j], s_dp[:n_upd, j], rtol=2e-5, atol=1e-6, err_msg=name)
    np.testing.assert_allclose(s1[:n_upd, 4], np.maximum(r0["stats"][:n_upd, 4], r1["stats"][:n_upd, 4]), rtol=1e-5)  # max_ratio
    d = np.abs(one - r0["params"])
    lr = c["lr"]
    # 12 Adam updates on gradients that agree to fp32 rounding: weights within 1e-6, except those whose gradient is ~0
    # (Adam normalises: such a weight may land a step apart); none further than the possible travel
    margins.lt(float((d > 1e-6).mean()), 0.005, f"fraction of weights > 1e-6 apart (max {d.max():.2e})")
    margins.leq(float(d.max()), 2.1 * lr * n_upd, "worst weight difference vs travel")


@pytest.mark.parametrize("env", [None, PEER])
def test_ppo_on_the_cnn_head_two_ranks_equal_one_learner_on_the_concatenated_batch(tmp_path, monkeypatch, env):
    """PPO on the convolutional engine (core/agent/ppo_cnn.py) as data-parallel learners: jh_ppo_loss_packed with the deferred critic -> the ranks' {sum e1, sum e2}
    -> jh_ppo_critic_select_strided -> backward -> gradient bucket mean -> clip + Adam.  Both ranks end with identical weights, and they are the weights of ONE
    learner on the two ranks' rows with the two ranks' minibatches side by side.  env PEER: everything through peer pointers, inside the learn() graph (three
    process() calls of the same rollout -- eager, capture + replay, replay; the weights move on, the LAST call's statistics are compared)."""
    ranks = _run_ranks("ppo_cnn", tmp_path, extra_env=env)
    r0, r1 = ranks
    assert np.array_equal(r0["params"], r1["params"]), "ranks diverged"
    assert np.array_equal(r0["grads"], r1["grads"])
    if env:
        assert int(r0["peer_timeouts"]) == 0 and int(r1["peer_timeouts"]) == 0 and int(r0["graphed"]) == 1
    c = W.PPO_CNN_CFG
    M, B, E, n_upd = c["W"] * c["T"], c["B"], c["E"], int(r0["n_upd"])
    agent = W.ppo_cnn_agent(2 * c["W"], 2 * B, use_graph=False)
    rows = [W.ppo_cnn_rows(0), W.ppo_cnn_rows(1)]
    cols = {k: np.concatenate([rows[0][k], rows[1][k]], 0) for k in rows[0]}
    perms = []
    for e in range(E):
        p0, p1 = r0["perms"][e], r1["perms"][e]
        perms.append(np.concatenate([np.concatenate([p0[o:o + B], M + p1[o:o + B]]) for o in range(0, M, B)]))
    from jorldy_amd import np_rng

    def fixed_lists(M_, E_, out):
        out.reshape(-1)[:] = np.concatenate(perms)
        return out

    monkeypatch.setattr(np_rng, "epoch_shuffles", fixed_lists)
    for _ in range(3 if env else 1):  # the ranks ran the same rollout that many times (eager, capture + replay, replay)
        agent.time_t = agent.learn_stamp = 0
        agent.process(cols, c["T"])
    monkeypatch.undo()
    torch.cuda.synchronize()
    s1 = npy(agent._static["stats"]).astype(np.float64)
    s_dp = 0.5 * (r0["stats"].astype(np.float64) + r1["stats"].astype(np.float64))
    np.testing.assert_array_equal(r0["stats"][:n_upd, 6:8], r1["stats"][:n_upd, 6:8])  # the same global c1 / c2 on both ranks, bit for bit
    gap = np.abs(s1[:n_upd, 6] - s1[:n_upd, 7]) / np.maximum(s1[:n_upd, 6], 1e-12)
    assert (gap > 1e-4).sum() >= 2, f"the value clamp never became active (relative |c1 - c2| per update: {gap})"
    tol = dict(rtol=2e-5, atol=1e-6) if not env else dict(rtol=2e-4, atol=1e-5)  # third learn() of two fp32 trajectories
    for j in (6, 7):
        np.testing.assert_allclose(s1[:n_upd, j], r0["stats"][:n_upd, j], err_msg="global c1 / c2 vs one learner", **tol)
    for j, name in ((1, "actor_loss"), (2, "critic_loss"), (3, "entropy_loss")):
        np.testing.assert_allclose(s1[:n_upd, j], s_dp[:n_upd, j], err_msg=name, **tol)
    d = np.abs(npy(agent._net.params) - r0["params"])
    n_all = n_upd * (3 if env else 1)
    margins.lt(float((d > 1e-5).mean()), 0.01, f"fraction of weights > 1e-5 apart (max {d.max():.2e})")
    margins.leq(float(d.max()), 2.1 * c["lr"] * n_all, "worst weight difference vs travel")


@pytest.mark.parametrize("mode,env", [("rainbow", None), ("rainbow", PEER), ("apex", None), ("apex", PEER)])
def test_value_learners_two_ranks_identical_weights_and_single_tree_is_weights(tmp_path, mode, env):
    """Rainbow and -- round 6, north_star's "Ape-X re-expressed as one learner per GPU" -- the Ape-X learner (dueling net, n-step double-Q,
    centered RMSprop, clip 40, PER shards with actor-side priorities), over the host-staged transport and through peer pointers."""
    r0, r1 = _run_ranks(mode, tmp_path, extra_env=env)
    if env:
        assert int(r0["peer_timeouts"]) == 0 and int(r1["peer_timeouts"]) == 0
    assert np.array_equal(r0["params"], r1["params"]), "ranks diverged"
    assert np.array_equal(r0["target"], r1["target"])
    assert not np.array_equal(r0["idx"], r1["idx"])  # they did sample different shards
    # (c) weights of ONE logical tree holding both shards, for the ranks' index lists (per_buffer.py:88-94)
    N = int(r0["N"])
    usp, beta = float(r0["usp"]), float(r0["beta"])
    roots = [float(r["tree_before"][0]) for r in (r0, r1)]
    counts = [int(r["count_before"]) for r in (r0, r1)]
    ROOT_, COUNT = roots[0] + roots[1], counts[0] + counts[1]
    ws = []
    for r in (r0, r1):
        p = r["tree_before"][r["idx"]]
        P = (1.0 - usp) * (p / ROOT_) + usp * (1.0 / COUNT)
        ws.append(((1.0 / COUNT) / P) ** beta)
    wmax = max(w.max() for w in ws)
    for r, w in zip((r0, r1), ws):
        np.testing.assert_allclose(r["w"], (w / wmax).astype(np.float32), rtol=2e-6)
    assert max(float(r0["w"].max()), float(r1["w"].max())) == pytest.approx(1.0, rel=1e-6)  # ONE sample of the global batch has weight 1
    assert np.all(np.isfinite(r0["losses"])) and np.all(np.isfinite(r1["losses"]))


@pytest.mark.parametrize("launcher,strong", [("torchrun", False), ("self", True)])
def test_bench_two_ranks_on_one_gpu_plumbing(tmp_path, launcher, strong):
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one process per rank) AND launching itself (`python bench.py
    --gpus 2` with no RANK in the environment: VERDICT r3 #4), backend gloo so that both ranks may share cuda:0: launch, per-rank pinning,
    attach_data_parallel (exact critic: two collectives per minibatch), barrier + max-over-ranks timing, one JSON line.  strong: the config's
    8 workers and minibatch of 256 split over the ranks (4 workers, 128 rows each)."""
    import json

    env = dict(os.environ, JH_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    args = ["--gpus", "2", "--full", "--steps", "3", "--warmup", "2", "--no-rainbow", "--no-roofline", "--no-cpu-baseline", "--hopper-iters", "1",
            "--apex-actors", "16", "--apex-updates", "240", "--apex-buffer", "200000", "--apex-prefill", "4000"] + (["--strong"] if strong else [])
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["config"]["parallelism"] == "dp2"
    assert out["scaling"] == ("strong" if strong else "weak") and out["config"]["workers_per_gpu"] == (4 if strong else 8) and out["config"]["batch_size"] == (128 if strong else 256)
    assert out["value"] > 0 and np.isfinite(out["last_result"]["critic_loss"]) and list(out)[-1] == "legs"
    ax = out["apex"]  # round 6: configs[3] as one learner + its actors + its replay shard per rank, gradients averaged per learn()
    assert "error" not in ax, ax
    assert ax["n_gpus"] == 2 and ax["value"] > 0 and ax["learner_updates_per_s"] > 0 and np.isfinite(ax["rank0"]["last_result"]["loss"])
    hp = out["hopper"]  # configs[4] strong-scaled over the two ranks: 16 workers and 1024 minibatch rows each, collector + DP learners
    assert hp["n_gpus"] == 2 and hp["config"]["workers_per_gpu"] == 16 and hp["config"]["batch_per_gpu"] == 1024 and hp["value"] > 0


def test_bench_two_ranks_prints_the_line_when_a_late_leg_hangs():
    """The N > 1 legs after the timed region sit under watchdogs (no multi-GPU box has ever run them): with the Ape-X leg's time limit set to a
    fraction of what it needs, rank 0 still prints the ONE line -- the timed PPO measurement intact, the leg an error entry -- and the job ends with rc 0."""
    import json

    env = dict(os.environ, JH_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", JH_APEX_DP_TIMEOUT="0.5")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--full", "--steps", "3", "--warmup", "2", "--no-rainbow", "--no-hopper", "--no-roofline", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and "did not finish in time" in out["apex"]["error"] and out["legs"]["ppo_env_transitions_s"] == out["value"]
