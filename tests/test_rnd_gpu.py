"""RND-PPO on the GPU: the entries of ops.RNDNet, jh_rnd_adv_mix and jh_rnd_ppo_loss_packed against the float64 truth of tests/rnd_truth.py
over its sweeps, with fp64_truth's criterion |ours - fp64| <= max(1e-5, 2 |torch-cpu-fp32 - fp64|) relative to the tensor's largest entry;
argument checks and determinism; the agent: graph replay against eager bit for bit, the learning rate that reaches only the policy's
optimizer, checkpoints in the reference's format, errors and the reference's configurations.

Dispatch boundaries of the new kernels, each with a case on both sides:
  rows per row lane   the batch-norm / moments kernels give a column 16 row lanes: b = 15, 16, 17; b = 2, 3 (fourteen / thirteen idle lanes)
  columns per group   16 columns a workgroup: H = 16 (one group), 32, 512; S = 2, 4, 11 in the moments kernel
  tile edges          the tile engine's 32-row tiles: b = 63, 64, 65, 257
  loss kernel         one workgroup of 1024 threads, a row per thread: b = 1, 2, 63 .. 65 (one wave | two), 256, 1024 (every thread a row)
  mix kernel          256 threads per row of n_step: T = 2, 8, 65, 128"""
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import rnd_truth as D
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

LR = 3e-3
F32 = torch.float32


def _net(cfg, max_batch, w, blk):
    from jorldy_amd import ops

    net = ops.RNDNet(cfg["S"], cfg["H"], cfg["W"], max_batch, "cuda", gamma_i=cfg["gamma_i"], obs_normalize=cfg["obs_norm"], ri_normalize=cfg["ri_norm"],
                     batch_norm=cfg["bn"])
    net.import_state({k: torch.from_numpy(v) for k, v in w.items()})
    net.set_stats(blk)
    net.set_hyper(LR, step=0)
    return net


def _bits(net):
    torch.cuda.synchronize()
    return b"".join(npy(t).tobytes() for t in (net.params, net.grads, net.m, net.v)) + b"".join(v.tobytes() for v in net.stats().values())


def _run_update(tag, cfg, b, max_norm):
    w, blk, s2, idx = D.update_case(tag, cfg, b)
    net = _net(cfg, max(b, 2), w, blk)
    stats = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    net.update(f32(s2), torch.from_numpy(idx).cuda(), max_norm, stats=stats)
    torch.cuda.synchronize()
    return net, npy(stats), s2[idx], w, blk


UPDATE_CASES = D.cases()


@pytest.mark.parametrize("tag,cfg,b", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_update_matches_float64(tag, cfg, b):
    """jh_rndnet_update against rnd_truth.update: the loss, the gradient of each of the predictor's tensors as it sits in the bucket after the
    step (clipped), the four batch norms' running statistics; everything else in the block, and every tensor of the target -- weights,
    gradients, moments --, bit-unchanged; the weights after the step as arithmetic (float64 Adam fed OUR clipped gradient lands on our
    weights).  Every other case clips (max_norm 0.02), the others do not (max_norm 50).

    b2 and b3 (a batch norm over two and three rows) are what the module's kernels normalise in double for (jh_curiosity.h: CUR_F64): with the
    float32 normalisation that ICM's instantiation keeps, b2's gradients sit 1.8e-4 of their largest entry from float64."""
    max_norm = 0.02 if len(tag) % 2 else 50.0
    net, stats, s2, w, blk = _run_update(tag, cfg, b, max_norm)
    t64, t32 = D.update(cfg, w, blk, s2, max_norm), D.update(cfg, w, blk, s2, max_norm, dtype=F32)
    assert stats[3] == 0.0 and stats[2] == 0.0 and stats[1] == 0.0, "the arrival mark"
    T.vs_exact(stats[:1], t64["loss"].reshape(1), t32["loss"].reshape(1), D.TOL, f"{tag} loss")
    assert (float(t64["norm"]) > max_norm) == (max_norm < 1.0), "the case clips exactly when it is meant to"
    grads = {k: npy(v) for k, v in net.export_state(net.grads).items()}
    for k in D.trainable(cfg):
        T.vs_exact(grads[k], t64["clipped"][k], t32["clipped"][k], D.TOL, f"{tag} d(loss)/d {k} after the clip")
    after = net.stats()
    for k in D.BLOCK_KEYS:
        if k.startswith("bn") and cfg["bn"]:
            T.vs_exact(after[k], t64["run"][k], t32["run"][k], D.TOL, f"{tag} {k}")
        else:
            assert after[k].tobytes() == np.asarray(blk[k], np.float32).tobytes(), f"{tag}: an update leaves {k} alone"
    w1 = {k: npy(v) for k, v in net.export_state().items()}
    moments = {k: (npy(m), npy(v)) for (k, m), (_, v) in zip(net.export_state(net.m).items(), net.export_state(net.v).items())}
    for k in w:
        if "target" in k:
            assert w1[k].tobytes() == w[k].tobytes() and not grads[k].any() and not moments[k][0].any() and not moments[k][1].any(), f"{tag}: the target's {k} is frozen"
    tr = D.trainable(cfg)
    T.check_first_step_from_our_gradient({k: w[k] for k in tr}, {k: grads[k] for k in tr}, {k: w1[k] for k in tr}, lambda ps: torch.optim.Adam(ps, lr=LR), LR, f"{tag} step")


REWARD_CASES = D.reward_cases()


@pytest.mark.parametrize("tag,cfg,M", REWARD_CASES, ids=[c[0] for c in REWARD_CASES])
def test_obs_update_and_reward_match_float64(tag, cfg, M):
    """jh_rndnet_obs_update + jh_rndnet_reward against rnd_truth.reward_pass: r_i before and after the normalisation, mean(r_i), every entry of
    the block; nothing written to the buckets."""
    w, blk, s2 = D.case_inputs(tag, cfg, M)
    net = _net(cfg, M, w, blk)
    before = b"".join(npy(t).tobytes() for t in (net.params, net.grads, net.m, net.v))
    ri_raw, ri, ri_mean = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(1, device="cuda")
    net.obs_update(f32(s2))
    net.reward(f32(s2), ri, ri_mean=ri_mean, ri_raw=ri_raw)
    torch.cuda.synchronize()
    t64, t32 = D.reward_pass(cfg, w, blk, s2), D.reward_pass(cfg, w, blk, s2, dtype=F32)
    for ours, k in ((ri_raw, "r_raw"), (ri, "r_i"), (ri_mean, "r_i_mean")):
        assert np.isfinite(npy(ours)).all()
        T.vs_exact(npy(ours), t64[k].reshape(-1), t32[k].reshape(-1), D.TOL, f"{tag} {k}")
    after = net.stats()
    for k in D.BLOCK_KEYS:
        if k.startswith("bn") and not cfg["bn"]:
            assert after[k].tobytes() == np.asarray(blk[k], np.float32).tobytes()
        else:
            T.vs_exact(after[k], t64["block"][k].reshape(-1), t32["block"][k].reshape(-1), D.TOL, f"{tag} {k}")
    assert b"".join(npy(t).tobytes() for t in (net.params, net.grads, net.m, net.v)) == before, "the no-grad pass writes no bucket"


def test_bad_sizes_are_refused_and_write_nothing():
    """JH_ERR_ARG before any launch: one row under batch norm, rows over max_batch, no row, a rollout the workers do not divide, one row for
    the moments, a hidden size that is no multiple of 4.  Buckets, block and outputs keep their bits."""
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    cfg = D.config(4, 16, W=3)
    w, blk, s2 = D.case_inputs("bad", cfg, 12)
    net = _net(cfg, 9, w, blk)
    before = _bits(net)
    S2, ri = f32(s2), torch.full((12,), -7.0, device="cuda")
    idx = lambda n: torch.arange(n, dtype=torch.int64, device="cuda")
    for n in (1, 10, 0):
        with pytest.raises(JhError, match="bad argument"):
            net.update(S2, idx(n), 1.0)
    with pytest.raises(JhError, match="bad argument"):
        net.reward(S2[:8].contiguous(), ri[:8])  # 8 rows, 3 workers
    with pytest.raises(JhError, match="bad argument"):
        net.reward(S2, ri)  # 12 rows > max_batch
    with pytest.raises(JhError, match="bad argument"):
        net.obs_update(S2[:1].contiguous())
    with pytest.raises(JhError, match="bad argument"):
        net.obs_update(S2)
    torch.cuda.synchronize()
    assert _bits(net) == before and bool((ri == -7.0).all())
    with pytest.raises(JhError):
        ops.RNDNet(4, 18, 1, 8, "cuda")
    with pytest.raises(JhError):
        ops.RNDNet(4, 16, 1, ops.RNDNet.MAX_BATCH + 1, "cuda")
    wp = D.random_weights(D.config(4, 16, W=3, bn=False), np.random.RandomState(0))
    plain = _net(D.config(4, 16, W=3, bn=False), 9, wp, blk)
    plain.update(S2, idx(1), 1.0)  # one row is fine without batch norm
    torch.cuda.synchronize()
    g = torch.zeros(4, 6, device="cuda")
    a = lambda *sh: torch.zeros(*sh, device="cuda")
    with pytest.raises(JhError, match="bad argument"):  # a row stride without room for v_i
        ops.rnd_ppo_loss_packed(a(4, 3), 2, None, a(4, 1), a(4), a(4), a(4), a(4), a(4), a(4, 1), 0.1, 0.5, 0.01, a(4, 3), a(8))
    with pytest.raises(JhError, match="bad argument"):  # one action
        ops.rnd_ppo_loss_packed(a(4, 6), 1, None, a(4, 1), a(4), a(4), a(4), a(4), a(4), a(4, 1), 0.1, 0.5, 0.01, g, a(8))
    torch.cuda.synchronize()
    assert not bool(g.any())


def test_param_count_equals_the_padded_sum_of_the_segments():
    from jorldy_amd import ops

    for bn in (True, False):
        net = ops.RNDNet(5, 20, 2, 8, "cuda", batch_norm=bn)
        up4 = lambda n: (n + 3) // 4 * 4
        assert net.n_params == sum(up4(r * c) for _, r, c in net.seg.values()) and len(net.seg) == (16 if bn else 8)
        assert net.n_train == sum(up4(r * c) for k, (_, r, c) in net.seg.items() if "predict" in k)
        assert [k for k, _ in net._pairs(net.params)] == list(D.shapes(D.config(5, 20, bn=bn)))


def test_two_identical_runs_give_identical_bits():
    for tag, cfg, b in (("det_b130", D.config(4, 48), 130), ("det_plain", D.config(5, 16, bn=False), 33)):
        runs = []
        for _ in range(2):
            net, stats, _, _, _ = _run_update(tag, cfg, b, 0.02)
            runs.append(_bits(net) + stats.tobytes())
        assert runs[0] == runs[1], tag
    cfg = D.config(4, 16, W=8)
    w, blk, s2 = D.case_inputs("det_reward", cfg, 1024)
    runs = []
    for _ in range(2):
        net, ri = _net(cfg, 1024, w, blk), torch.zeros(1024, device="cuda")
        net.obs_update(f32(s2))
        net.reward(f32(s2), ri)
        runs.append(_bits(net) + npy(ri).tobytes())
    assert runs[0] == runs[1]
    c = [c for c in D.loss_cases() if c[0] == "cont_A3_b1024_plain"][0]
    runs = [_run_loss(*c)[:2] for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---------------------------------------------------------------------------------------------- the loss and the mix
def _run_loss(tag, cont, A, b, variant):
    from jorldy_amd import ops

    x = D.loss_case(tag, cont, A, b, variant)
    heads = f32(x["heads"])
    grad = torch.full_like(heads, 9.0)
    stats = torch.full((8,), -1.0, device="cuda")
    ops.rnd_ppo_loss_packed(heads, A, None, f32(x["action"]), f32(x["adv"]), f32(x["ret"]), f32(x["ret_i"]), f32(x["v_old"]), f32(x["vi_old"]), f32(x["lp_old"]),
                            x["eps"], x["vf"], x["ent"], grad, stats, continuous=cont)
    torch.cuda.synchronize()
    return npy(grad), npy(stats), x


LOSS_CASES = D.loss_cases()


@pytest.mark.parametrize("tag,cont,A,b,variant", LOSS_CASES, ids=[c[0] for c in LOSS_CASES])
def test_ppo_loss_matches_float64(tag, cont, A, b, variant):
    """jh_rnd_ppo_loss_packed against rnd_truth.ppo_loss: the six statistics and the gradient in the heads' layout; the padding columns keep
    what they held."""
    grad, stats, x = _run_loss(tag, cont, A, b, variant)
    args = (cont, x["heads"], A, x["action"], x["adv"], x["ret"], x["ret_i"], x["v_old"], x["vi_old"], x["lp_old"], x["eps"], x["vf"], x["ent"])
    t64, t32 = D.ppo_loss(*args), D.ppo_loss(*args, dtype=F32)
    nv = (2 * A if cont else A) + 2
    assert stats[0] == 0.0 and stats[7] == 0.0
    for j, k in enumerate(("actor", "critic_e", "critic_i", "entropy", "max_ratio", "min_prob"), 1):
        T.vs_exact(stats[j : j + 1], torch.tensor([t64["stats"][k]], dtype=torch.float64), torch.tensor([t32["stats"][k]], dtype=torch.float64), D.TOL, f"{tag} {k}")
    T.vs_exact(grad[:, :nv], t64["grad"], t32["grad"], D.TOL, f"{tag} d(loss)/d(heads)")
    assert (grad[:, nv:] == 9.0).all(), "padding columns are not written"
    if variant == "critic":
        assert t64["means"]["c2"] > t64["means"]["c1"] and t64["means"]["i2"] > t64["means"]["i1"]
    if variant == "clipped":
        assert bool(((t64["rows"]["ratio"] < 1 - x["eps"]) | (t64["rows"]["ratio"] > 1 + x["eps"])).all())


def test_ppo_loss_reads_its_rows_through_the_index_list():
    from jorldy_amd import ops

    x = D.loss_case("idx", False, 3, 40, "plain")
    idx = np.random.RandomState(0).permutation(40)[:17].astype(np.int64)
    heads = f32(x["heads"][idx])
    g1, g2, s1, s2 = torch.zeros_like(heads), torch.zeros_like(heads), torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    rows = [f32(x[k]) for k in ("action", "adv", "ret", "ret_i", "v_old", "vi_old", "lp_old")]
    ops.rnd_ppo_loss_packed(heads, 3, torch.from_numpy(idx).cuda(), *rows, 0.1, 0.5, 0.01, g1, s1)
    ops.rnd_ppo_loss_packed(heads, 3, None, *[f32(x[k][idx]) for k in ("action", "adv", "ret", "ret_i", "v_old", "vi_old", "lp_old")], 0.1, 0.5, 0.01, g2, s2)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2) and torch.equal(s1, s2) and bool(g1.any())


@pytest.mark.parametrize("W,Tn", D.MIX_WT, ids=[f"W{w}_T{t}" for w, t in D.MIX_WT])
@pytest.mark.parametrize("episodic", [True, False], ids=["episodic", "non_episodic"])
@pytest.mark.parametrize("standardize", [True, False], ids=["std", "raw"])
def test_adv_mix_matches_float64(W, Tn, episodic, standardize):
    """Two jh_gae calls (standardize off; the intrinsic one with gamma_i and, non-episodic, a zero done column) + jh_rnd_adv_mix against
    rnd_truth.gae / adv_mix: both returns, their means and the mixed advantage."""
    from jorldy_amd import ops

    c = D.mix_case(W, Tn)
    M, gamma, gamma_i, lam, ext, intr = W * Tn, 0.99, 0.97, 0.95, 2.0, 0.7
    dev = {k: f32(v) for k, v in c.items()}
    zero = torch.zeros(M, device="cuda")
    out = {k: torch.zeros(M, device="cuda") for k in ("adv_e", "ret", "adv_i", "ret_i", "adv")}
    means = torch.zeros(8, device="cuda")
    ops.gae(dev["reward"], dev["done"], dev["v"], dev["vn"], Tn, gamma, lam, False, out=(out["adv_e"], out["ret"]))
    ops.gae(dev["r_i"], dev["done"] if episodic else zero, dev["vi"], dev["vin"], Tn, gamma_i, lam, False, out=(out["adv_i"], out["ret_i"]))
    ops.rnd_adv_mix(out["adv_e"], out["adv_i"], out["ret"], out["ret_i"], Tn, ext, intr, standardize, out["adv"], means)
    torch.cuda.synchronize()
    res = {}
    for dt in (torch.float64, F32):
        ae, re = D.gae(c["reward"], c["done"], c["v"], c["vn"], Tn, gamma, lam, True, dt)
        ai, ri = D.gae(c["r_i"], c["done"], c["vi"], c["vin"], Tn, gamma_i, lam, episodic, dt)
        res[dt] = dict(ret=re, ret_i=ri, adv=D.adv_mix(ae, ai, Tn, ext, intr, standardize, dt), means=torch.stack([re.mean(), ri.mean()]))
    tag = f"W{W}_T{Tn}_{'e' if episodic else 'n'}{'s' if standardize else 'r'}"
    for k in ("ret", "ret_i", "adv"):
        T.vs_exact(npy(out[k]), res[torch.float64][k], res[F32][k], D.TOL, f"{tag} {k}")
    T.vs_exact(npy(means[:2]), res[torch.float64]["means"], res[F32]["means"], D.TOL, f"{tag} means")
    assert not bool(means[2:].any())


# ---------------------------------------------------------------------------------------------- the agent
def _cols(trs):
    return {k: np.concatenate([t[k] for t in trs], 0) for k in ("state", "next_state", "reward", "done", "action")}


def _synthetic(S, A, M, cont, seed):
    from oracle import synth

    return _cols(synth.ppo_rollout(np.random.RandomState(seed), M, S, A, cont, clamp_every=0))


def _small_agent(cont, **over):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=5 if cont else 4, action_size=3 if cont else 2, hidden_size=32, network="continuous_policy_separate_value" if cont else "discrete_policy_separate_value",
              optim_config={"name": "adam", "lr": 1e-3}, batch_size=24, n_step=16, num_workers=4, run_step=10000, lr_decay=True, device="cuda",
              non_episodic=cont, use_standardization=cont)
    kw.update(over)
    agent = Agent("rnd_ppo", **kw)
    agent.memory.first_store = False
    return agent


def _learn(agent, cont, it, M=64, T_=16):
    r = agent.process(_synthetic(agent.state_size, agent.action_size, M, cont, 30 + it), (it + 1) * T_)
    torch.cuda.synchronize()
    return [r[k] for k in sorted(r)]


def _state(agent):
    n, i = agent._net, agent._rnd_net
    blk = np.concatenate([v.reshape(-1) for v in i.stats().values()])
    return torch.cat([n.params, n.m, n.v, i.params, i.m, i.v, torch.from_numpy(blk).cuda()]).clone()


RESULT_KEYS = {"actor_loss", "critic_e_loss", "critic_i_loss", "entropy_loss", "r_i", "max_ratio", "min_prob", "mean_ret", "mean_ret_i"}


@pytest.mark.parametrize("cont", [False, True])
def test_graph_replay_equals_eager_bit_for_bit_and_the_decay_reaches_the_policy_only(cont):
    """Three learns, eager vs warm-up + capture + replay: results, both buckets, both moment sets and the block are the same bits (and two
    identical runs give identical bits: the eager run is repeated).  Then the cosine decay reaches lr = 0: a replayed learn leaves the policy-
    value net unmoved and STILL moves the predictor."""
    Tn = 16
    out = []
    for use_graph in (False, False, True):
        torch.manual_seed(0)
        agent = _small_agent(cont, run_step=4 * Tn, use_graph=use_graph)
        np.random.seed(3)
        res = [_learn(agent, cont, it) for it in range(3)]
        out.append((res, _state(agent)))
        assert agent._rnd_steps == 27 and agent._rnd_batches == 30 and agent._adam_steps == 27
        if not use_graph:
            assert not agent._graphs
            continue
        assert agent._graphs, "learn() was captured"
        n_graphs = len(agent._graphs)
        _learn(agent, cont, 3)  # runs at the lr of step 3 Tn and leaves lr = 0 behind (cosine at step = run_step)
        assert agent._lr_now == pytest.approx(0.0, abs=1e-12)
        assert agent.rnd_optimizer.param_groups[0]["lr"] == 1e-3
        before = _state(agent)
        agent.lr_decay = False
        _learn(agent, cont, 4)
        after = _state(agent)
        n, ni = agent._net.n_params, agent._rnd_net.n_params
        assert torch.equal(after[:n], before[:n]), "lr 0: the policy-value net stays"
        assert not torch.equal(after[3 * n : 3 * n + ni], before[3 * n : 3 * n + ni]), "the module's Adam keeps its learning rate"
        assert len(agent._graphs) == n_graphs, "no new capture"
    assert np.isfinite(np.asarray(out[0][0])).all()
    assert np.array_equal(np.asarray(out[0][0]), np.asarray(out[1][0])) and torch.equal(out[0][1], out[1][1]), "two identical runs"
    assert np.array_equal(np.asarray(out[0][0]), np.asarray(out[2][0])), "results: replay vs eager"
    assert torch.equal(out[0][1], out[2][1]), "buckets, moments, block: replay vs eager"


@pytest.mark.parametrize("cont", [False, True])
def test_save_load_roundtrip_in_the_reference_format(cont, tmp_path):
    from jorldy_amd.core.network import Network

    torch.manual_seed(1)
    a = _small_agent(cont)
    np.random.seed(1)
    for it in range(2):
        assert np.isfinite(_learn(a, cont, it)).all()
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"network", "rnd", "optimizer", "rnd_optimizer"}
    heads = ["mu", "log_std"] if cont else ["pi"]
    assert list(ckpt["network"]) == [f"{m}.{t}" for m in ["head.l", "l"] + heads + ["v", "v_i"] for t in ("weight", "bias")]
    assert len(ckpt["rnd"]) == 35 and list(ckpt["rnd"])[:9] == ["rms_obs.mean", "rms_obs.var", "rms_obs.count", "rms_ri.mean", "rms_ri.var", "rms_ri.count", "rff.rewems",
                                                                 "fc1_predict_mlp.weight", "fc1_predict_mlp.bias"]
    assert int(ckpt["rnd"]["bn2_target_mlp.num_batches_tracked"]) == 2 * (1 + 3 * 3) and float(ckpt["rnd"]["rms_obs.count"]) == pytest.approx(128.0001, rel=1e-6)
    # torch's Adam skips the parameters that never get a gradient (the seven buffer-like ones and the target's eight): state for the predictor's eight only
    assert sorted(ckpt["rnd_optimizer"]["state"]) == [7, 8, 9, 10, 15, 16, 17, 18] and len(ckpt["rnd_optimizer"]["param_groups"][0]["params"]) == 23
    # plain torch modules and optimizers built from the containers take all four entries
    m = Network("rnd_mlp", a.state_size, a.action_size, 4, 0.99, D_hidden=32)
    m.load_state_dict(ckpt["rnd"])
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    opt.load_state_dict(ckpt["rnd_optimizer"])
    assert float(opt.state[m.fc1_predict_mlp.weight]["step"]) == a._rnd_steps == 18 and m.fc1_target_mlp.weight not in opt.state
    assert torch.equal(opt.state[m.bn2_predict_mlp.bias]["exp_avg"], a._rnd_views[-1][1].cpu())
    pv = Network(a.network._net.kind == "pv2" and "discrete_policy_separate_value" or "continuous_policy_separate_value", a.state_size, a.action_size, D_hidden=32)
    pv.load_state_dict(ckpt["network"])
    popt = torch.optim.Adam(pv.parameters(), lr=1e-3)
    popt.load_state_dict(ckpt["optimizer"])
    assert float(popt.state[pv.v_i.weight]["step"]) == a._adam_steps == 18
    blk = a._rnd_net.stats()
    assert np.array_equal(m.rff.rewems.detach().numpy(), blk["rff.rewems"]) and np.array_equal(m.bn1_target_mlp.running_var.numpy(), blk["bn1_target_mlp.running_var"])
    torch.manual_seed(2)
    b = _small_agent(cont)
    b.load(str(tmp_path))
    torch.cuda.synchronize()
    assert torch.equal(_state(b), _state(a)) and b._rnd_steps == a._rnd_steps and b._rnd_batches == a._rnd_batches and b._adam_steps == a._adam_steps
    np.random.seed(7)
    want = [_learn(a, cont, it) for it in (2, 3)]
    np.random.seed(7)
    got = [_learn(b, cont, it) for it in (2, 3)]
    assert np.array_equal(np.asarray(got), np.asarray(want)) and torch.equal(_state(b), _state(a)), "a loaded agent continues bit for bit"


def test_save_full_load_full_resumes_bit_for_bit(tmp_path):
    torch.manual_seed(1)
    a = _small_agent(False)
    np.random.seed(1)
    for it in range(2):
        _learn(a, False, it)
    a.save_full(str(tmp_path))
    want = [_learn(a, False, it) for it in (2, 3)]
    torch.manual_seed(5)
    np.random.seed(99)
    b = _small_agent(False)
    b.load_full(str(tmp_path))
    assert b.time_t == 32 and b._adam_steps == 18 and b._rnd_steps == 18 and b._rnd_batches == 20
    got = [_learn(b, False, it) for it in (2, 3)]
    assert np.array_equal(np.asarray(got), np.asarray(want)), "two further learns after load_full vs the uninterrupted agent"
    assert torch.equal(_state(b), _state(a))


def test_one_seed_gives_the_mirrors_initial_weights_and_act_returns_the_action_only():
    from jorldy_amd.core.network import Network

    for cont in (False, True):
        torch.manual_seed(11)
        a = _small_agent(cont)
        torch.manual_seed(11)
        net = Network("continuous_policy_separate_value" if cont else "discrete_policy_separate_value", a.state_size, a.action_size, D_hidden=32)
        rnd = Network("rnd_mlp", a.state_size, a.action_size, 4, 0.99, D_hidden=32)
        for k, v in net.state_dict().items():
            assert torch.equal(a.network.state_dict()[k].cpu(), v), k
        for k, v in rnd.state_dict().items():
            assert torch.equal(a.rnd.state_dict()[k].cpu(), v), k
        x = np.random.RandomState(0).randn(6, a.state_size).astype(np.float32)
        for training in (True, False):
            out = a.act(x, training)
            assert set(out) == {"action"} and out["action"].shape == (6, a.action_size if cont else 1)


def test_errors():
    a = _small_agent(False, batch_size=21)  # 64 rows: minibatches of 21, 21, 21 and ONE
    with pytest.raises(ValueError, match="ONE row"):
        a.process(_synthetic(4, 2, 64, False, 1), 16)
    a = _small_agent(False, num_workers=5)
    with pytest.raises(ValueError, match="num_workers"):
        a.process(_synthetic(4, 2, 64, False, 1), 16)
    a = _small_agent(False, num_workers=1, n_step=1)
    with pytest.raises(ValueError, match="more than one row"):
        a.process(_synthetic(4, 2, 1, False, 1), 1)
    with pytest.raises(NotImplementedError):
        a._capture_targets(64)
    with pytest.raises(NotImplementedError):
        a.process_begin(16)
    with pytest.raises(NotImplementedError):
        a.process_end()
    assert not a.early_ready()
    a.grad_sync = object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        a.learn()


COMMON = dict(head="mlp", n_step=128, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, clip_grad_norm=1.0, lr_decay=True, rnd_network="rnd_mlp", gamma_i=0.99,
              extrinsic_coeff=2.0, intrinsic_coeff=1.0, obs_normalize=True, ri_normalize=True, batch_norm=True, run_step=100000, device="cuda",
              optim_config={"name": "adam", "lr": 1e-4})
DISCRETE = dict(network="discrete_policy_separate_value", gamma=0.99, batch_size=64, vf_coef=0.5, num_workers=8)
CONFIGS = [("cartpole", dict(DISCRETE, state_size=4, action_size=2, ent_coef=0.01, use_standardization=False, non_episodic=False)),
           ("mountaincar", dict(DISCRETE, state_size=2, action_size=3, ent_coef=0.0)),
           ("pong_mlagent", dict(DISCRETE, state_size=8, action_size=3, ent_coef=0.0)),
           ("mujoco_hopper", dict(network="continuous_policy_separate_value", state_size=11, action_size=3, gamma=0.999, batch_size=32, vf_coef=1.0, ent_coef=0.001,
                                  use_standardization=False, num_workers=64))]


@pytest.mark.parametrize("label,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_reference_config_constructs_acts_and_learns_once(label, kw):
    """config.rnd_ppo.cartpole / .mountaincar / .pong_mlagent / .mujoco as they stand (hidden 512, 8 x 128 rows in minibatches of 64; mujoco: 64 x
    128 rows in minibatches of 32 on Hopper's sizes)."""
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    agent = Agent("rnd_ppo", **COMMON, **kw)
    assert agent._rnd_net.H == 512 and len(list(agent.rnd.parameters())) == 23 and len(agent.rnd.state_dict()) == 35
    agent.memory.first_store = False
    cont = kw["network"].startswith("continuous")
    assert set(agent.act(np.zeros((8, kw["state_size"]), np.float32))) == {"action"}
    M = 128 * kw["num_workers"]
    n_upd = 3 * (M // kw["batch_size"])
    r = agent.process(_synthetic(kw["state_size"], kw["action_size"], M, cont, 1), 128)
    torch.cuda.synchronize()
    assert set(r) == RESULT_KEYS and all(np.isfinite(v) for v in r.values()), r
    assert agent._adam_steps == n_upd and agent._rnd_steps == n_upd and agent._rnd_batches == n_upd + 1 and r["r_i"] > 0 and r["critic_i_loss"] > 0


# ---------------------------------------------------------------------------------------------- the agent against the fixtures
FIX_TOL = dict(rtol=1e-5, atol=1e-5)  # the project's fixture tolerance


def _agent_for(fx, **over):
    from jorldy_amd.core.agent import Agent

    kw = D.agent_kwargs(fx.spec)
    kw.update(device="cuda")
    kw.update(over)
    torch.manual_seed(fx.init_seed)
    agent = Agent("rnd_ppo", **kw)
    init = ({k: npy(v) for k, v in agent.network.state_dict().items()}, {k: npy(v) for k, v in agent.rnd.state_dict().items()})
    agent.network.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx.sd0.items()})
    agent.rnd.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx.rnd0.items()})
    agent._sync_rnd_in()
    agent.memory.first_store = False
    return agent, init


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name):
    """Both learns of the fixture on ONE agent (the second continues from the first's end: rms_obs, rms_ri, rewems, the four running statistics,
    both Adam steps) with the recorded numpy seed.  At rtol and atol 1e-5: the initial weights under the fixture's torch seed,
    the same index lists, the pre-pass tensors (r_i, v, v_i, adv, ret, ret_i, log pi_old), every minibatch's five losses, the result, the
    statistics block after the learn (the running means carry the fc biases in front of them, which travel by Adam's steps on rounding
    noise: the weights' cap) and num_batches_tracked = 1 + n_upd per learn; the last minibatch's gradients of both networks as they sit in the
    buckets and both Adam moments of both networks; the end weights of BOTH networks within the caps of the other agents' fixture tests: at most
    0.5 % of entries further than 2e-5 from the reference's, the worst within 2.1 lr."""
    fx = D.load_fixture(name)
    z = fx.z
    agent, init = _agent_for(fx)
    if not fx.recipe:
        for sd, prefix in zip(init, ("init/", "init_rnd/")):
            for k, v in sd.items():
                np.testing.assert_allclose(v, z[prefix + k], **FIX_TOL, err_msg=f"{name} initial {k}")
    nmb = fx.n_minibatch()
    for k in range(fx.learns):
        np.random.seed(int(z[f"l{k}/np_seed"]))
        result = agent.process(_cols(fx.rollout(k)), (k + 1) * fx.T)
        torch.cuda.synchronize()
        st = agent._static
        assert set(result) == RESULT_KEYS
        assert np.array_equal(npy(st["idx"][: fx.spec["n_epoch"] * fx.M]), np.concatenate([z[f"l{k}/mb{i}/idx"] for i in range(nmb)])), "other index lists were drawn"
        M = fx.M
        for ours, key in ((st["r_i"], "r_i"), (st["v"][:M], "value"), (st["v_i"][:M], "v_i"), (st["adv"], "adv"), (st["ret"], "ret"), (st["ret_i"], "ret_i"),
                          (st["logp_old"], "log_prob_old")):
            np.testing.assert_allclose(npy(ours).reshape(-1), z[f"l{k}/pre/{key}"].reshape(-1), **FIX_TOL, err_msg=f"{name} l{k} pre-pass {key}")
        s, r = npy(st["stats"]).astype(np.float64), npy(st["rnd_stats"]).astype(np.float64)
        for i in range(nmb):
            for ours, key in ((s[i, 1], "actor_loss"), (s[i, 2], "critic_e_loss"), (s[i, 3], "critic_i_loss"), (s[i, 4], "entropy_loss"), (r[i, 0], "rnd_loss")):
                np.testing.assert_allclose(ours, float(z[f"l{k}/mb{i}/{key}"]), **FIX_TOL, err_msg=f"{name} l{k} mb{i} {key}")
        for key in sorted(result):
            np.testing.assert_allclose(result[key], float(z[f"l{k}/result/{key}"]), rtol=1e-3 if key in ("max_ratio", "min_prob") else 1e-5, atol=1e-5, err_msg=f"l{k} result {key}")
        assert agent._adam_steps == agent._rnd_steps == (k + 1) * nmb
        last = nmb - 1
        for tag, net in (("grad", agent._net), ("rnd_grad", agent._rnd_net)):
            rec = fx.sub(f"l{k}/mb{last}/{tag}/")
            ours = {kk: npy(v) for kk, v in net.export_state(net.grads).items()}
            for kk, v in rec.items():
                np.testing.assert_allclose(fx.thin(ours[kk]).reshape(-1), v.reshape(-1), **FIX_TOL, err_msg=f"{name} l{k} mb{last} {tag} {kk}")
        agent._sync_rnd_out()
        rsd = {key: npy(v) for key, v in agent.rnd.state_dict().items()}
        ref_rnd = fx.sub(f"l{k}/rnd1/")
        assert list(rsd) == list(ref_rnd)
        for key in rsd:
            if key.split(".")[0] in ("rms_obs", "rms_ri", "rff") or "running" in key:
                np.testing.assert_allclose(fx.thin(rsd[key]).reshape(-1), ref_rnd[key].reshape(-1), rtol=1e-5, atol=2.1 * fx.lr if "running_mean" in key else 1e-5,
                                           err_msg=f"l{k} block {key}")
            elif key.endswith("num_batches_tracked"):
                assert int(rsd[key]) == int(ref_rnd[key]) == (k + 1) * (1 + nmb)
        psd = {key: npy(v) for key, v in agent.network.state_dict().items()}
        wsd = {key: rsd[key] for key in D.shapes(fx.cfg)}
        # a linear layer's bias in front of a batch norm has an exactly zero gradient: Adam turns the rounding noise left there into steps of up to
        # lr each, in the reference as here, so those entries are held to their own travel cap alone and left out of the count of far entries
        noise = {f"{l}_predict_mlp.bias" for l in ("fc1", "fc2")} if fx.spec["on"] else set()
        for tag, sd, ref in (("policy-value net", psd, fx.sub(f"l{k}/sd1/")), ("module", wsd, ref_rnd)):
            tot = bad = worst = 0.0
            for kk in sd:
                dd = np.abs(fx.thin(np.asarray(sd[kk], dtype=np.float64)).reshape(-1) - np.asarray(ref[kk], dtype=np.float64).reshape(-1))
                if kk in noise:  # up to lr per Adam step in either run, so up to 2 lr apart per step taken so far (2.1 as below: 2 x 1.05)
                    margins.leq(float(dd.max()) / fx.lr, 2.1 * (k + 1) * nmb, f"{name} l{k} {tag} {kk}: difference / lr vs the possible travel of a zero-gradient bias")
                else:
                    worst = max(worst, float(dd.max()) / fx.lr)
                if kk not in noise:
                    n = float(np.asarray(sd[kk]).size)
                    tot, bad = tot + n, bad + float((dd > 2e-5).sum()) * n / dd.size
            margins.leq(bad / tot, 0.005, f"{name} l{k} {tag}: fraction of weights further than 2e-5 from the reference's")
            margins.leq(worst, 2.1, f"{name} l{k} {tag}: worst weight difference / lr vs the possible travel")
        for tag, net, names, prefix in (("policy", agent._net, list(psd), "opt1"), ("module", agent._rnd_net, D.trainable(fx.cfg), "rnd_opt1")):
            for bucket, mname in ((net.m, "exp_avg"), (net.v, "exp_avg_sq")):
                ours, ref = {kk: npy(v) for kk, v in net.export_state(bucket).items()}, fx.sub(f"l{k}/{prefix}/{mname}/")
                assert sorted(ref) == sorted(names), f"{tag}: the reference's optimizer holds state for exactly these"
                for kk in names:
                    np.testing.assert_allclose(fx.thin(ours[kk]).reshape(-1), ref[kk].reshape(-1), **FIX_TOL, err_msg=f"{name} l{k} {tag} {mname} {kk}")
            assert int(z[f"l{k}/{prefix}/step"]) == (k + 1) * nmb
        for key, p in agent.rnd.named_parameters():
            assert bool(int(z[f"l{k}/rnd_opt1/has_state/{key}"])) == (key in D.trainable(fx.cfg)), key
        assert {kk for kk, _ in agent._rnd_net._pairs(agent._rnd_net.m, True)} == set(D.trainable(fx.cfg))


# ---------------------------------------------------------------------------------------------- learning curve
def _hip_curve(seed):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    c = D.CURVE_CONFIG
    W, Tn = c["workers"], c["n_step"]
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = Agent("rnd_ppo", run_step=c["run_step"], num_workers=W, device="cuda", seed=seed, **c["agent"])
    agent.memory.first_store = False
    env = ops.CartPoleVec(W, seed=1000 + seed)
    curve, step = [], 0
    S, N = np.empty((Tn, W, 4), np.float32), np.empty((Tn, W, 4), np.float32)
    Aa, R, Dn = np.empty((Tn, W, 1), np.float32), np.empty((Tn, W, 1), np.float32), np.empty((Tn, W, 1), np.float32)
    for _ in range(c["iterations"]):
        for t in range(Tn):
            S[t] = env.obs()
            a = agent.act(S[t], True)["action"]
            nxt, rew, done = env.step(a)
            N[t], Aa[t], R[t, :, 0], Dn[t, :, 0] = nxt, np.asarray(a, dtype=np.float32).reshape(W, 1), rew, done
        wm = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2).reshape(W * Tn, -1))  # worker-major, as the reference's sync mode concatenates its actors
        curve.append(W * Tn / max(1, int(Dn.sum())))
        step += Tn
        agent.process({"state": wm(S), "action": wm(Aa), "reward": wm(R), "next_state": wm(N), "done": wm(Dn)}, step)
    return curve


def test_cartpole_learning_curve_tracks_the_real_reference():
    """config.rnd_ppo.cartpole, 8 workers x 128 steps x 40 iterations on ops.CartPoleVec, seeds 1-3, against the curves of the UNMODIFIED reference
    agent on the oracle's CartPole (tests/golden/curves_reference_rnd_ppo.json, tools/gen_golden_rnd.py).  ICM's criterion with the margin taken
    from the fixture: both sides gain at least 3x from the first iteration to the mean of the last five, and the HIP end (mean episode length
    over the last five iterations, averaged over the seeds) lies within the reference's own seed spread (the largest minus the smallest of its
    three seeds' ends) of the reference's end."""
    import json

    with open(os.path.join(D.GOLDEN, "curves_reference_rnd_ppo.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_rnd.py --only curves"
    ref = fx["rnd_ppo_cartpole"]["reference"]
    r_end, spread = D.curve_criterion(ref)
    hip = [_hip_curve(s) for s in D.CURVE_CONFIG["seeds"]]
    g_end, g_gain = float(np.mean([D.curve_end(c) for c in hip])), [D.curve_end(c) / c[0] for c in hip]
    with open(os.path.join(os.path.dirname(margins.dump()), "learning_curve_rnd_ppo_cartpole.json"), "w") as f:
        json.dump({"config": fx["config"], "metric": fx["metric"], "hip": hip, "reference": ref, "hip_end": g_end, "reference_end": r_end, "reference_spread": spread,
                   "hip_gain": g_gain}, f)
    print(f"RND-PPO CartPole: HIP ends {[D.curve_end(c) for c in hip]}, mean {g_end:.1f}, gains {g_gain}; reference end {r_end:.1f}, seed spread {spread:.1f}")
    assert all(np.isfinite(c).all() for c in hip)
    assert min(g_gain) >= 3.0, "every seed learns: the last five iterations over the first"
    margins.leq(abs(g_end - r_end), spread, "rnd_ppo: |end of the HIP curves - end of the reference's| vs the reference's seed spread")
