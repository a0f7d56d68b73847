"""ICM-PPO on the GPU: the entries of ops.ICMNet against the float64 truth of tests/icm_truth.py over the sweeps of icm_truth.cases() and
icm_truth.reward_cases(), argument checks and determinism; the agent: graph replay against eager bit for bit and the learning rate that reaches
only PPO's optimizer, checkpoints in the reference's format, errors, the reference's configurations, every learn of the fixtures of
tools/gen_golden_icm.py, and the CartPole learning curve against the unmodified reference's.

Dispatch boundaries of the new kernels, each with a case on both sides:
  rows per row lane   the batch-norm / moments kernels give a column 16 row lanes (r, r + 16, ...): b = 15, 16, 17 (a lane without a row, one row
                      each, a lane with two), b = 2, 3 (fourteen / thirteen idle lanes)
  columns per group   16 columns a workgroup: H = 16 (one group), H = 48 (three); S = 3, 4, 17 in the moments kernel (a partial group, two groups)
  tile edges          the tile engine's 32-row tiles: b = 31, 32, 33, 63, 64, 65, 130 (2b rows in the trunk: 62 .. 260); forward_fc1 / forward_fc2
                      with an odd row length (discrete: 257, H + 1) and with 256 + A, H + A (continuous A = 1, 3, 19)
  reward kernel       one thread a worker, 256 threads: W = 1, 5, 8 and W = 257 (a thread with two workers); T = 2 .. 128"""
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import icm_truth as D
import margins
from tests.util import f32, npy

pytestmark = pytest.mark.gpu

LR = 3e-3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(cfg, max_batch, w, blk):
    from jorldy_amd import ops

    net = ops.ICMNet(cfg["S"], cfg["H"], cfg["A"], cfg["cont"], cfg["W"], max_batch, "cuda", eta=cfg["eta"], gamma=cfg["gamma"], obs_normalize=cfg["obs_norm"],
                     ri_normalize=cfg["ri_norm"], batch_norm=cfg["bn"])
    net.import_state({k: torch.from_numpy(v) for k, v in w.items()})
    net.set_stats(blk)
    net.set_hyper(LR, step=0)
    return net


def _bits(net):
    torch.cuda.synchronize()
    return b"".join(npy(t).tobytes() for t in (net.params, net.grads, net.m, net.v)) + b"".join(v.tobytes() for v in net.stats().values())


def _run_update(tag, cfg, b, max_norm):
    """One update on b rows picked by an index list out of a longer rollout.  -> (net, stats [4], the rows' inputs, weights, block)"""
    w, blk, s, a, s2, idx = D.update_case(tag, cfg, b)
    net = _net(cfg, max(b, 2), w, blk)
    stats = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    net.update(f32(s), f32(s2), f32(a), torch.from_numpy(idx).cuda(), 0.2, max_norm, stats=stats)
    torch.cuda.synchronize()
    return net, npy(stats), (s[idx], a[idx], s2[idx]), w, blk


UPDATE_CASES = D.cases()


@pytest.mark.parametrize("tag,cfg,b", UPDATE_CASES, ids=[c[0] for c in UPDATE_CASES])
def test_update_matches_float64(tag, cfg, b):
    """jh_icmnet_update against icm_truth.update in float64: both losses (icm_truth.bound("loss")), the gradient of every segment as it sits in
    the bucket after the step -- clipped, relative to the segment's largest entry (bound("grad"); four times the float32 comparator's measured
    error where batch norm runs over two rows) --, the batch norms' running statistics (bound("block")), everything else in the block
    bit-unchanged, and the weights after the step as arithmetic: float64 Adam fed OUR clipped gradient from the case's weights lands on our
    weights (fp64_truth's per-element criterion).  Every other case clips (max_norm 0.02), the others do not (max_norm 50)."""
    max_norm = 0.02 if len(tag) % 2 else 50.0
    net, stats, (s, a, s2), w, blk = _run_update(tag, cfg, b, max_norm)
    t64 = D.update(cfg, w, blk, s, a, s2, 0.2, max_norm)
    assert stats[3] == 0.0 and stats[2] == 0.0, "the arrival mark"
    for j, k in enumerate(("l_f", "l_i")):
        assert np.isfinite(stats[j])
        margins.leq(abs(float(stats[j]) - float(t64[k])) / abs(float(t64[k])), D.bound("loss"), f"{tag} {k} |ours - fp64| / |fp64|")
    assert (float(t64["norm"]) > max_norm) == (max_norm < 1.0), "the case clips exactly when it is meant to"
    grads = {k: npy(v) for k, v in net.export_state(net.grads).items()}
    assert list(grads) == list(t64["clipped"])
    for k, e in D.grad_errors(cfg, grads, t64["clipped"]).items():
        margins.leq(e, D.bound(D.grad_class(cfg, b)), f"{tag} d(loss)/d {k} after the clip, / max |fp64|")
    after = net.stats()
    for k in D.BLOCK_KEYS:
        if k.startswith("bn") and cfg["bn"]:
            margins.leq(D.rel(after[k], t64["run"][k]), D.bound("block"), f"{tag} {k}")
        else:
            assert after[k].tobytes() == np.asarray(blk[k], np.float32).tobytes(), f"{tag}: an update leaves {k} alone"
    w1 = {k: npy(v) for k, v in net.export_state().items()}
    T.check_first_step_from_our_gradient(w, grads, w1, lambda ps: torch.optim.Adam(ps, lr=LR), LR, f"{tag} step")
    assert float(npy(net.m).std()) > 0 and float(npy(net.v).max()) > 0


REWARD_CASES = D.reward_cases()


@pytest.mark.parametrize("tag,cfg,M", REWARD_CASES, ids=[c[0] for c in REWARD_CASES])
def test_obs_update_and_reward_match_float64(tag, cfg, M):
    """jh_icmnet_obs_update + jh_icmnet_reward against icm_truth.reward_pass in float64: r_i before and after the normalisation, the mixed
    reward and mean(r_i) (bound("r_i")), every entry of the block (bound("block")), nothing written to the buckets.  The filter's aliasing is
    visible: rms_ri.var from the per-step filter states would miss the recorded one by more than 1e-3 wherever T > 1 states differ."""
    w, blk, s, a, s2, r = D.case_inputs(tag, cfg, M)
    net = _net(cfg, M, w, blk)
    before = b"".join(npy(t).tobytes() for t in (net.params, net.grads, net.m, net.v))
    reward, ri_raw, ri, ri_mean = f32(r), torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda"), torch.zeros(1, device="cuda")
    net.obs_update(f32(s2))
    net.reward(f32(s), f32(s2), f32(a), reward, 0.7, 1.3, ri_mean=ri_mean, ri_raw=ri_raw, ri=ri)
    torch.cuda.synchronize()
    t64 = D.reward_pass(cfg, w, blk, s, a, s2, r, 0.7, 1.3)
    for ours, k in ((ri_raw, "r_raw"), (ri, "r_i"), (reward, "reward")):
        assert np.isfinite(npy(ours)).all()
        margins.leq(D.rel(npy(ours), t64[k]), D.bound("r_i"), f"{tag} {k} / max |fp64|")
    margins.leq(abs(float(ri_mean) - float(t64["r_i_mean"])) / abs(float(t64["r_i_mean"])), D.bound("r_i"), f"{tag} mean(r_i)")
    after = net.stats()
    for k in D.BLOCK_KEYS:
        if k.startswith("bn") and not cfg["bn"]:
            assert after[k].tobytes() == np.asarray(blk[k], np.float32).tobytes()
        else:
            margins.leq(D.rel(after[k], t64["block"][k]), D.bound("block"), f"{tag} {k}")
    Tn = M // cfg["W"]
    if Tn >= 8:
        _, v_true, _ = D.moments_merge(blk["rms_ri.mean"], blk["rms_ri.var"], blk["rms_ri.count"], t64["true_stack"].reshape(-1, 1))
        assert abs(float(v_true) - float(t64["block"]["rms_ri.var"])) > 1e-3 * float(t64["block"]["rms_ri.var"]), "the aliasing is visible in this case"
        assert abs(float(after["rms_ri.var"]) - float(t64["block"]["rms_ri.var"])) < 0.01 * abs(float(v_true) - float(t64["block"]["rms_ri.var"]))
    assert b"".join(npy(t).tobytes() for t in (net.params, net.grads, net.m, net.v)) == before, "the no-grad pass writes no bucket"


def test_bad_sizes_are_refused_and_write_nothing():
    """JH_ERR_ARG before any launch: one row under batch norm, rows over max_batch, a rollout the workers do not divide, one row for the moments,
    an action size outside the policy's range.  Buckets and block keep their bits."""
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    cfg = D.config(4, 2, 16, False, W=3)
    w, blk, s, a, s2, r = D.case_inputs("bad", cfg, 12)
    net = _net(cfg, 9, w, blk)
    before = _bits(net)
    S, S2, A, R = f32(s), f32(s2), f32(a), f32(r)
    idx = lambda n: torch.arange(n, dtype=torch.int64, device="cuda")
    with pytest.raises(JhError, match="bad argument"):
        net.update(S, S2, A, idx(1), 0.2, 1.0)
    with pytest.raises(JhError, match="bad argument"):
        net.update(S, S2, A, idx(10), 0.2, 1.0)
    with pytest.raises(JhError, match="bad argument"):
        net.update(S, S2, A, idx(0), 0.2, 1.0)
    with pytest.raises(JhError, match="bad argument"):
        net.reward(S[:8].contiguous(), S2[:8].contiguous(), A[:8].contiguous(), R[:8].contiguous())  # 8 rows, 3 workers
    with pytest.raises(JhError, match="bad argument"):
        net.reward(S, S2, A, R)  # 12 rows > max_batch
    with pytest.raises(JhError, match="bad argument"):
        net.obs_update(S2[:1].contiguous())
    with pytest.raises(JhError, match="bad argument"):
        net.obs_update(S2)
    torch.cuda.synchronize()
    assert npy(R).tobytes() == r.tobytes() and _bits(net) == before
    for cont, A_bad in ((False, 40), (True, 20), (False, 0)):
        with pytest.raises(JhError):
            ops.ICMNet(4, 16, A_bad, cont, 1, 8, "cuda")
    with pytest.raises(JhError):
        ops.ICMNet(4, 16, 2, False, 1, ops.ICMNet.MAX_BATCH + 1, "cuda")
    plain = _net(D.config(4, 2, 16, False, W=3, bn=False), 9, {k: v for k, v in w.items() if not k.startswith("bn")}, blk)
    plain.update(S, S2, A, idx(1), 0.2, 1.0)  # one row is fine without batch norm
    torch.cuda.synchronize()


def test_two_identical_runs_give_identical_bits():
    for tag, cfg, b in (("det_b130", D.config(4, 2, 48, False), 130), ("det_cont", D.config(5, 3, 16, True), 33)):
        runs = []
        for _ in range(2):
            net, stats, _, _, _ = _run_update(tag, cfg, b, 0.02)
            runs.append(_bits(net) + stats.tobytes())
        assert runs[0] == runs[1], tag
    cfg = D.config(4, 2, 16, False, W=8)
    w, blk, s, a, s2, r = D.case_inputs("det_reward", cfg, 1024)
    runs = []
    for _ in range(2):
        net, reward = _net(cfg, 1024, w, blk), f32(r)
        net.obs_update(f32(s2))
        net.reward(f32(s), f32(s2), f32(a), reward)
        runs.append(_bits(net) + npy(reward).tobytes())
    assert runs[0] == runs[1]


# ---------------------------------------------------------------------------------------------- the agent
def _cols(trs):
    return {k: np.concatenate([t[k] for t in trs], 0) for k in ("state", "next_state", "reward", "done", "action")}


def _synthetic(S, A, M, cont, seed):
    from oracle import synth

    return _cols(synth.ppo_rollout(np.random.RandomState(seed), M, S, A, cont, clamp_every=0))


def _small_agent(cont, **over):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=5 if cont else 4, action_size=3 if cont else 2, hidden_size=32, network="continuous_policy_value" if cont else "discrete_policy_value",
              optim_config={"name": "adam", "lr": 1e-3}, batch_size=24, n_step=16, num_workers=4, run_step=10000, lr_decay=True, eta=0.1, device="cuda")
    kw.update(over)
    agent = Agent("icm_ppo", **kw)
    agent.memory.first_store = False
    return agent


def _learn(agent, cont, it, M=64, T_=16):
    r = agent.process(_synthetic(agent._net.S, agent._net.A, M, cont, 30 + it), (it + 1) * T_)
    torch.cuda.synchronize()
    return [r[k] for k in sorted(r)]


def _state(agent):
    n, i = agent._net, agent._icm_net
    blk = np.concatenate([v.reshape(-1) for v in i.stats().values()])
    return torch.cat([n.params, n.m, n.v, i.params, i.m, i.v, torch.from_numpy(blk).cuda()]).clone()


RESULT_KEYS = {"actor_loss", "critic_loss", "entropy_loss", "max_ratio", "min_prob", "mean_ret", "r_i", "l_f", "l_i"}


@pytest.mark.parametrize("cont", [False, True])
def test_graph_replay_equals_eager_bit_for_bit_and_the_decay_reaches_ppo_only(cont):
    """Three learns, eager vs warm-up + capture + replay: results, both buckets, both moment sets and the block are the same bits.  Then the cosine
    decay reaches lr = 0: a replayed learn leaves the policy-value net unmoved and STILL moves the ICM net (learning_rate_decay reaches
    self.optimizer only, base.py:103-104)."""
    Tn = 16
    out = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent = _small_agent(cont, run_step=4 * Tn, use_graph=use_graph)
        np.random.seed(3)
        res = [_learn(agent, cont, it) for it in range(3)]
        out.append((res, _state(agent)))
        assert agent._icm_steps == 27 and agent._icm_batches == 30 and agent._adam_steps == 27
        if not use_graph:
            assert not agent._graphs
            continue
        assert agent._graphs, "learn() was captured"
        n_graphs = len(agent._graphs)
        _learn(agent, cont, 3)  # runs at the lr of step 3 Tn and leaves lr = 0 behind (cosine at step = run_step)
        assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(0.0, abs=1e-12)
        assert agent.icm_optimizer.param_groups[0]["lr"] == 1e-3
        before = _state(agent)
        agent.lr_decay = False
        _learn(agent, cont, 4)
        after = _state(agent)
        n, ni = agent._net.n_params, agent._icm_net.n_params
        assert torch.equal(after[:n], before[:n]), "lr 0: the policy-value net stays"
        assert not torch.equal(after[3 * n : 3 * n + ni], before[3 * n : 3 * n + ni]), "the ICM's Adam keeps its learning rate"
        assert len(agent._graphs) == n_graphs, "no new capture"
    assert np.array_equal(np.asarray(out[0][0]), np.asarray(out[1][0])), "results: replay vs eager"
    assert torch.equal(out[0][1], out[1][1]), "buckets, moments, block: replay vs eager"


@pytest.mark.parametrize("cont", [False, True])
def test_save_load_roundtrip_in_the_reference_format(cont, tmp_path):
    from jorldy_amd.core.network import Network

    torch.manual_seed(1)
    a = _small_agent(cont)
    np.random.seed(1)
    for it in range(2):
        r = _learn(a, cont, it)
        assert np.isfinite(r).all()
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"network", "icm", "optimizer", "icm_optimizer"}
    assert len(ckpt["icm"]) == 34 and list(ckpt["icm"])[:9] == ["rms_obs.mean", "rms_obs.var", "rms_obs.count", "rms_ri.mean", "rms_ri.var", "rms_ri.count", "rff.rewems",
                                                                 "fc1.weight", "fc1.bias"]
    assert int(ckpt["icm"]["bn2.num_batches_tracked"]) == 2 * (1 + 3 * 3) and float(ckpt["icm"]["rms_obs.count"]) == pytest.approx(128.0001, rel=1e-6)
    # torch's Adam skips the seven parameters that never get a gradient: state for 7 .. 24 only
    assert sorted(ckpt["icm_optimizer"]["state"]) == list(range(7, 25)) and len(ckpt["icm_optimizer"]["param_groups"][0]["params"]) == 25
    # a plain torch module and optimizer built from the container take both
    m = Network("icm_mlp", a._net.S, a._net.A, 4, 0.99, 0.1, "continuous" if cont else "discrete", D_hidden=32)
    m.load_state_dict(ckpt["icm"])
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    opt.load_state_dict(ckpt["icm_optimizer"])
    assert float(opt.state[m.fc1.weight]["step"]) == a._icm_steps == 18 and m.rms_obs.mean not in opt.state
    assert torch.equal(opt.state[m.bn1_next.bias]["exp_avg"], a._icm_views[-1][1].cpu())
    blk = a._icm_net.stats()
    assert np.array_equal(m.rff.rewems.detach().numpy(), blk["rff.rewems"]) and np.array_equal(m.bn1.running_var.numpy(), blk["bn1.running_var"])
    torch.manual_seed(2)
    b = _small_agent(cont)
    b.load(str(tmp_path))
    torch.cuda.synchronize()
    assert torch.equal(_state(b), _state(a)) and b._icm_steps == a._icm_steps and b._icm_batches == a._icm_batches and b._adam_steps == a._adam_steps
    np.random.seed(7)
    want = [_learn(a, cont, it) for it in (2, 3)]
    np.random.seed(7)
    got = [_learn(b, cont, it) for it in (2, 3)]
    assert np.array_equal(np.asarray(got), np.asarray(want)) and torch.equal(_state(b), _state(a)), "a loaded agent continues bit for bit"


def test_save_full_load_full_resumes_bit_for_bit(tmp_path):
    """The reference's "icm" entry carries the whole block, so save_full needs nothing beyond the two step counters of its manifest."""
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
    assert b.time_t == 32 and b._adam_steps == 18 and b._icm_steps == 18 and b._icm_batches == 20
    got = [_learn(b, False, it) for it in (2, 3)]
    assert np.array_equal(np.asarray(got), np.asarray(want)), "two further learns after load_full vs the uninterrupted agent"
    assert torch.equal(_state(b), _state(a))


def test_switches_are_honoured_when_off():
    """obs_normalize, ri_normalize and batch_norm each False: the state_dict loses the batch norms' 15 keys, the block's moments still follow
    (the reference updates them whatever the switches say), and a learn is finite."""
    torch.manual_seed(0)
    np.random.seed(0)
    a = _small_agent(False, obs_normalize=False, ri_normalize=False, batch_norm=False)
    assert len(a.icm.state_dict()) == 19 and len(list(a.icm.parameters())) == 19
    r = _learn(a, False, 0)
    assert np.isfinite(r).all()
    blk = a._icm_net.stats()
    assert float(blk["rms_obs.count"]) == pytest.approx(64.0001, rel=1e-6) and float(blk["rms_ri.count"]) == pytest.approx(64.0001, rel=1e-6)


def test_errors():
    a = _small_agent(False, batch_size=21)  # 64 rows: minibatches of 21, 21, 21 and ONE
    with pytest.raises(ValueError, match="ONE row"):
        a.process(_synthetic(4, 2, 64, False, 1), 16)
    a = _small_agent(False, num_workers=5)
    with pytest.raises(ValueError, match="num_workers"):
        a.process(_synthetic(4, 2, 64, False, 1), 16)
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


CONFIGS = [("cartpole", dict(state_size=4, action_size=2, network="discrete_policy_value", eta=0.1, optim_config={"name": "adam", "lr": 2.5e-4})),
           ("mountaincar", dict(state_size=2, action_size=3, network="discrete_policy_value", eta=0.1, optim_config={"name": "adam", "lr": 2.5e-4})),
           ("pong_mlagent", dict(state_size=8, action_size=3, network="discrete_policy_value", eta=0.1, optim_config={"name": "adam", "lr": 2.5e-4})),
           ("continuous_S11_A3", dict(state_size=11, action_size=3, network="continuous_policy_value", eta=0.01, optim_config={"name": "adam", "lr": 5e-4}))]


@pytest.mark.parametrize("label,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_reference_config_constructs_and_learns_once(label, kw):
    """config.icm_ppo.cartpole / .mountaincar / .pong_mlagent as they stand (hidden 512, 8 x 128 rows, batch 32, 3 epochs) and a continuous setup."""
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    agent = Agent("icm_ppo", head="mlp", gamma=0.99, batch_size=32, n_step=128, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, clip_grad_norm=1.0,
                  use_standardization=False, lr_decay=True, icm_network="icm_mlp", beta=0.2, lamb=1.0, extrinsic_coeff=1.0, intrinsic_coeff=1.0, run_step=100000,
                  num_workers=8, device="cuda", **kw)
    assert agent._icm_net.H == 512 and len(list(agent.icm.parameters())) == 25 and len(agent.icm.state_dict()) == 34
    agent.memory.first_store = False
    cont = kw["network"].startswith("continuous")
    r = agent.process(_synthetic(kw["state_size"], kw["action_size"], 1024, cont, 1), 128)
    torch.cuda.synchronize()
    assert set(r) == RESULT_KEYS and all(np.isfinite(v) for v in r.values()), r
    assert agent._adam_steps == 96 and agent._icm_steps == 96 and agent._icm_batches == 97 and r["r_i"] > 0 and r["l_f"] > 0


# ---------------------------------------------------------------------------------------------- the agent against the fixtures
def _agent_for(fx, **over):
    from jorldy_amd.core.agent import Agent

    kw = fx.agent_kwargs()
    kw.update(device="cuda")
    kw.update(over)
    agent = Agent("icm_ppo", **kw)
    agent.network.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx.sd0.items()})
    agent.icm.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx.icm0.items()})
    agent._sync_icm_in()
    agent.memory.first_store = False
    return agent


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name, monkeypatch):
    """Every learn of the fixture on ONE agent (the second continues from the first's end: rms_obs, rms_ri, rewems, the running statistics, both
    Adam steps) with the recorded numpy seed: the same index lists; the mixed reward, r_i and PPO's pre-pass (rtol and atol 1e-5); every
    minibatch's l_f / l_i within max(1e-5, four times the drift of the reference's own float32 losses from the float64 chain, which the
    generator recorded) and PPO's three losses (rtol and atol 1e-5, as PPO's own fixture tests); result keys and values; the whole block after the
    learn (rtol 1e-5, atol 1e-6; the two running means that carry fc1.bias: the weights' cap); the end weights of BOTH networks within the caps of the other agents' fixture tests: at most 0.5 % of
    entries further than 2e-5 from the reference's, the worst within 2.1 lr."""
    fx = D.load_fixture(name)
    z = fx.z
    monkeypatch.setenv("JH_PPO_PREDRAW", "0")  # the lists are drawn inside learn(): st["idx"] still holds THIS learn's afterwards
    agent = _agent_for(fx)
    nmb = fx.n_minibatch()
    for k in range(fx.learns):
        np.random.seed(int(z[f"l{k}/np_seed"]))
        cols = _cols(fx.rollout(k))
        result = agent.process(cols, (k + 1) * fx.T)
        torch.cuda.synchronize()
        st = agent._static
        assert set(result) == RESULT_KEYS
        assert np.array_equal(npy(st["idx"][: fx.n_epoch * fx.M]), np.concatenate([z[f"l{k}/mb{i}/idx"] for i in range(nmb)])), "other index lists were drawn"
        pre = fx.sub(f"l{k}/pre/")
        mixed = npy(st["tr"]["reward"]).reshape(-1)
        np.testing.assert_allclose(mixed, pre["reward"].reshape(-1), rtol=1e-5, atol=1e-5, err_msg=f"l{k} mixed reward")
        np.testing.assert_allclose(mixed - cols["reward"].reshape(-1).astype(np.float32), z[f"l{k}/r_i"].reshape(-1), rtol=1e-5, atol=2e-5, err_msg=f"l{k} r_i out of the mix")
        for ours, key in ((st["value"], "value"), (st["next_value"], "next_value")):
            np.testing.assert_allclose(npy(ours).reshape(-1), pre[key].reshape(-1), rtol=1e-5, atol=1e-5, err_msg=f"l{k} pre-pass {key}")
        loss_tol = max(1e-5, 4.0 * float(z[f"l{k}/truth_loss_dev"]))
        icm_stats, ppo_stats = npy(st["icm_stats"][:nmb]).astype(np.float64), npy(agent._stats[:nmb]).astype(np.float64)
        for i in range(nmb):
            for j, key in enumerate(("l_f", "l_i")):
                margins.leq(abs(icm_stats[i, j] - float(z[f"l{k}/mb{i}/{key}"])) / abs(float(z[f"l{k}/mb{i}/{key}"])), loss_tol, f"{name} l{k} mb{i} {key}")
            for j, key in ((1, "actor_loss"), (2, "critic_loss"), (3, "entropy_loss")):
                np.testing.assert_allclose(ppo_stats[i, j], float(z[f"l{k}/mb{i}/{key}"]), rtol=1e-5, atol=1e-5, err_msg=f"l{k} mb{i} {key}")
        for key in sorted(result):
            tol = 1e-3 if key in ("max_ratio", "min_prob") else 1e-5
            print(f"{name} l{k} result {key}: ours {result[key]!r} reference {float(z[f'l{k}/result/{key}'])!r}")
            np.testing.assert_allclose(result[key], float(z[f"l{k}/result/{key}"]), rtol=tol, atol=1e-5, err_msg=f"l{k} result {key}")
        assert agent._adam_steps == agent._icm_steps == (k + 1) * nmb
        agent._export_optim_state()
        agent._sync_icm_out()
        isd = {key: npy(v) for key, v in agent.icm.state_dict().items()}
        ref_icm = fx.sub(f"l{k}/icm1/")
        assert list(isd) == list(ref_icm)
        for key in isd:
            if key.split(".")[0] in ("rms_obs", "rms_ri", "rff") or "running" in key:
                # fc1.bias sits in front of bn1 and bn1_next: its exact gradient is zero, Adam turns the rounding noise left there into steps of up to
                # lr each, and the two running means that contain it travel with it -- they get the weights' own cap (2.1 lr) instead
                atol = 2.1 * fx.lr if key in ("bn1.running_mean", "bn1_next.running_mean") else 1e-6
                np.testing.assert_allclose(fx.thin(isd[key]).reshape(-1), ref_icm[key].reshape(-1), rtol=1e-5, atol=atol, err_msg=f"l{k} block {key}")
            elif key.endswith("num_batches_tracked"):
                assert int(isd[key]) == int(ref_icm[key]) == (k + 1) * (1 + nmb)
        psd = {key: npy(v) for key, v in agent.network.state_dict().items()}
        for tag, sd, ref, sizes in (("policy-value net", psd, fx.sub(f"l{k}/sd1/"), {key: v.size for key, v in psd.items()}),
                                    ("ICM", {key: isd[key] for key in D.shapes(fx.cfg)}, ref_icm, {key: np.prod(sh) for key, sh in D.shapes(fx.cfg).items()})):
            frac, worst = D.weight_caps(fx, sd, ref, sizes)
            margins.leq(frac, 0.005, f"{name} l{k} {tag}: fraction of weights further than 2e-5 from the reference's")
            margins.leq(worst, 2.1, f"{name} l{k} {tag}: worst weight difference / lr vs the possible travel")
        for key, p in agent.icm.named_parameters():
            has = bool(int(z[f"l{k}/icm_opt1/has_state/{key}"]))
            assert (p in agent.icm_optimizer.state and bool(agent.icm_optimizer.state[p])) == has == p.requires_grad, key


# ---------------------------------------------------------------------------------------------- learning curve
def _hip_curve(seed):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    c = D.CURVE_CONFIG
    W, Tn = c["workers"], c["n_step"]
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = Agent("icm_ppo", run_step=c["run_step"], num_workers=W, device="cuda", seed=seed, **c["agent"])
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
    """config.icm_ppo.cartpole, 8 workers x 128 steps x 40 iterations on ops.CartPoleVec, seeds 1-3, against the curves of the UNMODIFIED reference
    agent on the oracle's CartPole (tests/golden/curves_reference_icm_ppo.json, tools/gen_golden_icm.py).  V-MPO's test criterion: both sides gain
    at least 3x from the first iteration to the mean of the last five, and the HIP end (mean episode length over the last five iterations,
    averaged over the seeds) lies within a factor 2 of the reference's."""
    import json

    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_icm_ppo.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_icm.py --only curves"
    ref = fx["icm_ppo_cartpole"]["reference"]
    hip = [_hip_curve(s) for s in D.CURVE_CONFIG["seeds"]]
    g_gain, r_gain = [D.curve_gain(c) for c in hip], [D.curve_gain(c) for c in ref]
    g_end, r_end = float(np.mean([np.mean(c[-5:]) for c in hip])), float(np.mean([np.mean(c[-5:]) for c in ref]))
    # the curves go beside the margin ledger (the scratch directory tests/margins.py writes to), before anything is asserted
    margins.record(max(g_end / r_end, r_end / g_end), 2.0, "icm_ppo: end of the HIP curves vs end of the reference's, as a factor")
    with open(os.path.join(os.path.dirname(margins.dump()), "learning_curve_icm_ppo_cartpole.json"), "w") as f:
        json.dump({"config": fx["config"], "metric": fx["metric"], "hip": hip, "reference": ref, "hip_gain": g_gain, "reference_gain": r_gain, "hip_end": g_end,
                   "reference_end": r_end}, f)
    print(f"ICM-PPO CartPole: HIP gains {g_gain}, end {g_end:.1f}; reference gains {r_gain}, end {r_end:.1f}")
    assert all(np.isfinite(c).all() for c in hip)
    assert min(g_gain) >= 3.0 and min(r_gain) >= 3.0, "both learn: the last five iterations over the first"
    assert 0.5 * r_end <= g_end <= 2.0 * r_end
