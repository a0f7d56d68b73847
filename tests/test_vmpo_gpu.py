"""V-MPO on the GPU: the loss kernels against the float64 truth of tests/vmpo_truth.py over every block size the launch takes and every corner of
the top-half selection, the multipliers' device-side Adam step as arithmetic, determinism and argument checks; the agent against the reference's
fixtures (tools/gen_golden_vmpo.py), graph replay against eager bit for bit, checkpoints, the reference's configurations, and the CartPole
learning curve against the unmodified reference's."""
import json
import os

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins
import vmpo_truth as D
from tests.util import cu, f32, npy

pytestmark = pytest.mark.gpu

TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the loss kernels
def _run_kernel(cont, c, has_state=(True, True, True), want_mask=True):
    """-> (grads {head: array}, stats [8], block after (ops.vmpo_block_read), mask [b], raw block before, raw block after)"""
    from jorldy_amd import ops

    b = c["idx"].size
    blk = ops.vmpo_block(*[float(x) for x in c["mult"]], *[float(x) for x in c["floors"]], *D.EPS_DEFAULT, m=c["m"], v=c["v"], has_state=has_state)
    blk[:3] = f32(c["mult"])  # exactly the case's values (vmpo_block raises them to the floors, which the cases already respect)
    before = npy(blk).copy()
    hyper = ops.vmpo_hyper(D.LR, D.BETAS[0], D.BETAS[1], D.ADAM_EPS, D.STEP0)
    mask = torch.full((b,), -1.0, dtype=torch.float32, device="cuda") if want_mask else None
    idx = cu(c["idx"])
    if cont:
        g_mu, g_ls, g_v, stats = ops.vmpo_loss_continuous(f32(c["mu_raw"]), f32(c["log_std_raw"]), f32(c["v_pred"]), idx, f32(c["action"]), f32(c["adv"]), f32(c["value_old"]),
                                                          f32(c["mu_raw_old"]), f32(c["log_std_raw_old"]), blk, hyper, mask=mask)
        grads = {"mu_raw": npy(g_mu), "log_std_raw": npy(g_ls), "v": npy(g_v)}
    else:
        g_z, g_v, stats = ops.vmpo_loss_discrete(f32(c["logits"]), f32(c["v_pred"]), idx, f32(c["action"]), f32(c["adv"]), f32(c["value_old"]), f32(c["logits_old"]), blk, hyper,
                                                 mask=mask)
        grads = {"logits": npy(g_z), "v": npy(g_v)}
    torch.cuda.synchronize()
    return grads, npy(stats).copy(), ops.vmpo_block_read(blk), (npy(mask) if want_mask else None), before, npy(blk).copy()


def _scalar(ours, exact, ref32, what):
    """|ours - exact| / |exact| <= max(TOL, 2 x the float32 reference's own error); a float32 reference that is inf or NaN (the `hot` cases) leaves TOL."""
    scale = abs(exact) + 1e-30
    e_ref = abs(ref32 - exact) / scale if np.isfinite(ref32) else 0.0
    margins.leq(abs(float(ours) - exact) / scale, max(TOL, 2.0 * e_ref), f"{what} |ours - fp64| / |fp64| (reference fp32: {e_ref:.2e})")


CASES = [(False, A, b) for A in D.DISCRETE_A for b in D.LOSS_B] + [(True, A, b) for A in D.CONTINUOUS_A for b in D.LOSS_B]


@pytest.mark.parametrize("cont,A,b", CASES, ids=[f"{'cont' if c else 'disc'}-A{A}-b{b}" for c, A, b in CASES])
def test_loss_kernel_matches_float64(cont, A, b):
    """Every variant at one (policy, A, b): top-half membership EXACTLY the truth's (the optional mask output), head gradients by
    fp64_truth.grad_vs_exact at TOL, each loss within max(TOL, 2 x the float32 reference's own error), the multipliers' recorded gradients against the magnitude of their terms, and their step as arithmetic: float64 Adam fed the block's OWN recorded
    gradient lands on the block's new value (fp64_truth's per-element bound), moments at 1e-5.  Discrete: alpha_sigma and its moments are bit-unchanged."""
    for variant in D.VARIANTS:
        if variant == "clamped" and not cont:
            continue
        what = f"{'cont' if cont else 'disc'} A{A} b{b} {variant}"
        c = D.case(cont, b, A, variant)
        t64, t32 = D.case_truth(cont, c), D.case_truth(cont, c, torch.float32)
        grads, stats, blk, mask, raw0, raw1 = _run_kernel(cont, c, has_state=(True, True, False))
        assert np.array_equal(mask == 1.0, t64["top"]) and np.isin(mask, (0.0, 1.0)).all(), f"{what}: top-half membership"
        if variant == "all_equal" or b < 2:
            assert not t64["top"].any()
        ref32_ok = all(np.isfinite(g).all() for g in t32["grads"].values())
        for k, g in grads.items():
            assert np.isfinite(g).all(), f"{what}: d {k}"
            T.grad_vs_exact(g, t64["grads"][k], t32["grads"][k] if ref32_ok else None, TOL, f"{what} d(loss)/d {k}")
        if variant == "hot":
            assert not np.isfinite(t32["eta_loss"]), "float32 torch overflows here"
        empty = not t64["top"].any()
        for j, key in enumerate(("actor", "critic", "eta_loss", "alpha_loss")):
            if key == "eta_loss" and empty:
                assert np.isnan(stats[2]) and np.isnan(t64["eta_loss"]), f"{what}: eta_loss of an empty top half is NaN, as in the reference"
                continue
            assert np.isfinite(stats[j]), f"{what}: {key}"
            _scalar(stats[j], t64[key], t32[key], f"{what} {key}")
        n_mult = 3 if cont else 2
        for j in range(n_mult):
            n = D.NAMES[j]
            g = blk[n]["grad"]
            if j == 0 and empty:
                assert np.isnan(g) and np.isnan(blk[n]["value"]) and np.isnan(stats[4]), f"{what}: eta after an empty top half is NaN (fmaxf would have hidden it)"
                continue
            e_ref = abs(t32["mult_grads"][j] - t64["mult_grads"][j]) / t64["mult_scale"][j] if np.isfinite(t32["mult_grads"][j]) else 0.0
            margins.leq(abs(g - t64["mult_grads"][j]) / t64["mult_scale"][j], max(TOL, 2.0 * e_ref), f"{what} d(loss)/d {n} against the magnitude of its terms")
            x0 = float(c["mult"][j])
            w, m, v = D.multiplier_step(x0, g, c["m"][j], c["v"][j], D.STEP0, D.LR, c["floors"][j], D.BETAS, D.ADAM_EPS)
            margins.leq(abs(blk[n]["value"] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * D.LR, f"{what} {n} after float64 Adam on OUR gradient")
            margins.leq(abs(blk[n]["m"] - m), 1e-5 * abs(m), f"{what} {n} exp_avg")
            margins.leq(abs(blk[n]["v"] - v), 1e-5 * abs(v), f"{what} {n} exp_avg_sq")
            assert blk[n]["has_state"] and stats[4 + j] == np.float32(blk[n]["value"])
            if variant == "floor":
                assert blk[n]["value"] == float(c["floors"][j]), f"{what}: {n} is clamped to its floor"
        if not cont:
            for off in (2, 5, 8, 17, 20):  # value, exp_avg, exp_avg_sq, has-state flag, last gradient of alpha_sigma
                assert raw0[off].tobytes() == raw1[off].tobytes(), f"{what}: a discrete policy leaves alpha_sigma's block entry {off} untouched"
            assert not blk["alpha_sigma"]["has_state"] and stats[6] == c["mult"][2]
        assert stats[7] == 0.0 and raw0[9:15].tobytes() == raw1[9:15].tobytes()


def test_single_row_minibatch_has_an_empty_top_half_and_no_fault():
    """b = 1: nothing above the only row's median.  No actor gradient, the critic's and the KL's gradients are the truth's, eta turns NaN."""
    for cont, A in ((False, 2), (True, 3)):
        c = D.case(cont, 1, A, "plain")
        t64 = D.case_truth(cont, c)
        grads, stats, blk, mask, _, _ = _run_kernel(cont, c)
        assert mask.tolist() == [0.0] and not t64["top"].any() and stats[0] == 0.0 and np.isnan(stats[2]) and np.isnan(blk["eta"]["value"])
        for k, g in grads.items():
            T.grad_vs_exact(g, t64["grads"][k], None, TOL, f"b 1 d(loss)/d {k}")
        assert np.isfinite(blk["alpha_mu"]["value"])


def test_kernels_are_bit_identical_across_runs_and_reject_bad_sizes():
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    for cont, A in ((False, 6), (True, 17)):
        for b in (257, 1024):
            c = D.case(cont, b, A, "ties")
            r1, r2 = _run_kernel(cont, c), _run_kernel(cont, c)
            for k in r1[0]:
                assert r1[0][k].tobytes() == r2[0][k].tobytes(), (cont, b, k)
            assert r1[1].tobytes() == r2[1].tobytes() and r1[5].tobytes() == r2[5].tobytes() and r1[3].tobytes() == r2[3].tobytes()
    blk, hyper = ops.vmpo_block(), ops.vmpo_hyper(1e-3)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    for b, A in ((0, 2), (1025, 2), (4, 0)):
        M = max(b, 1)
        with pytest.raises(JhError, match="bad argument"):
            ops.vmpo_loss_discrete(z(b, A), z(b), torch.zeros(b, dtype=torch.int64, device="cuda"), z(M, 1), z(M), z(M), z(M, max(A, 1)), blk, hyper)
        with pytest.raises(JhError, match="bad argument"):
            ops.vmpo_loss_continuous(z(b, A), z(b, A), z(b), torch.zeros(b, dtype=torch.int64, device="cuda"), z(M, max(A, 1)), z(M), z(M), z(M, max(A, 1)), z(M, max(A, 1)),
                                     blk, hyper)
    torch.cuda.synchronize()
    assert npy(blk).tobytes() == npy(ops.vmpo_block()).tobytes(), "a refused call leaves the block alone"


# ---------------------------------------------------------------------------------------------- the agent against the fixtures
def _agent_for(fx, **over):
    from jorldy_amd.core.agent import Agent

    kw = fx.agent_kwargs()
    kw.update(device="cuda")
    kw.update(over)
    agent = Agent("vmpo", **kw)
    agent.network.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in fx.sd0.items()})
    agent.memory.first_store = False
    return agent


def _cols(trs):
    return {k: np.concatenate([t[k] for t in trs], 0) for k in ("state", "next_state", "reward", "done", "action")}


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name, monkeypatch):
    """Every learn of the fixture on ONE agent (the second continues from the first's end, multipliers included) with the recorded numpy seed:
    the same index lists; the pre-pass (old heads, values, advantages: rtol and atol 1e-5); every minibatch's four losses (rtol 1e-5) and
    multipliers after their step (fp64_truth's per-element bound around the reference's value), their moments (2e-5); result keys; end weights
    within the caps of the other agents' fixture tests (at most 0.5 % further than 2e-5 from the reference's, the worst within 2.1 lr)."""
    fx = D.load_fixture(name)
    z = fx.z
    monkeypatch.setenv("JH_PPO_PREDRAW", "0")  # the lists are drawn inside learn(): st["idx"] still holds THIS learn's afterwards, not the next one's drawn ahead
    agent = _agent_for(fx)
    nmb = fx.n_minibatch()
    names = ("mu_raw", "log_std_raw") if fx.cont else ("logits",)
    for k in range(fx.learns):
        np.random.seed(int(z[f"l{k}/np_seed"]))
        result = agent.process(_cols(fx.rollout(k)), (k + 1) * fx.T)
        torch.cuda.synchronize()
        st = agent._static
        assert set(result) == {"actor_loss", "critic_loss", "eta_loss", "alpha_loss", "eta", "alpha_mu", "alpha_sigma"}
        assert np.array_equal(npy(st["idx"][: fx.M]), np.concatenate([fx.mb(k, i)["idx"] for i in range(nmb)])), "other index lists were drawn"
        pre = fx.pre(k)
        for ours, key in [(st["h0"], names[0]), (st["value"], "value"), (st["adv"], "adv")] + ([(st["h1"], names[1])] if fx.cont else []):
            np.testing.assert_allclose(npy(ours).reshape(-1), pre[key].reshape(-1), rtol=1e-5, atol=1e-5, err_msg=f"l{k} pre-pass {key}")
        stats = npy(agent._stats[:nmb]).astype(np.float64)
        for i in range(nmb):
            mb = fx.mb(k, i)
            for j, key in enumerate(("actor_loss", "critic_loss", "eta_loss", "alpha_loss")):
                print(f"{name} l{k} mb{i} {key}: ours {stats[i, j]!r} reference {float(mb[key])!r}")
                np.testing.assert_allclose(stats[i, j], float(mb[key]), rtol=1e-5, err_msg=f"l{k} mb{i} {key}")
            for j, n in enumerate(D.NAMES):
                x0, w = float(mb[f"mult0/{n}"]), float(mb[f"mult1/{n}"])
                print(f"{name} l{k} mb{i} {n}: ours {stats[i, 4 + j]!r} reference {w!r}")
                margins.leq(abs(stats[i, 4 + j] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - x0) + 1e-6 * fx.lr, f"l{k} mb{i} {n} after its step")
        for key in sorted(result):
            np.testing.assert_allclose(result[key], float(z[f"l{k}/result/{key}"]), rtol=1e-5, err_msg=f"l{k} result {key}")
        blk = agent.multipliers()
        last = fx.mb(k, nmb - 1)
        for j, n in enumerate(D.NAMES):
            assert blk[n]["value"] == result[n] and blk[n]["has_state"] == bool(int(last[f"mult1/{n}/has_state"]))
            if blk[n]["has_state"]:
                np.testing.assert_allclose(blk[n]["m"], float(last[f"mult1/{n}/exp_avg"]), rtol=2e-5, atol=1e-9, err_msg=f"l{k} {n} exp_avg")
                np.testing.assert_allclose(blk[n]["v"], float(last[f"mult1/{n}/exp_avg_sq"]), rtol=2e-5, err_msg=f"l{k} {n} exp_avg_sq")
        assert agent._adam_steps == (k + 1) * nmb
        sd = {key: npy(v) for key, v in agent.network.state_dict().items()}
        tot = bad = 0
        worst = 0.0
        for key, v in sd.items():
            dd = np.abs(fx.thin(v) - z[f"l{k}/sd1/{key}"])
            tot += dd.size
            bad += int((dd > 2e-5).sum())
            worst = max(worst, float(dd.max()) / fx.lr)
        margins.leq(bad / tot, 0.005, f"l{k} fraction of weights further than 2e-5 from the reference's")
        margins.leq(worst, 2.1, f"l{k} worst weight difference / lr vs the possible travel")
    if name == "vmpo_continuous":
        assert float(npy(agent._stats[0])[5]) == np.float32(fx.floors[1]), "the first step of alpha_mu is clamped to its floor"


# ---------------------------------------------------------------------------------------------- graph replay, learning rate
def _state(agent):
    n = agent._net
    return torch.cat([n.params, n.m, n.v, agent._mult]).clone()


def _synthetic(S, A, M, cont, seed):
    from oracle import synth

    return _cols(synth.ppo_rollout(np.random.RandomState(seed), M, S, A, cont, clamp_every=0))


@pytest.mark.parametrize("cont", [False, True])
def test_graph_replay_equals_eager_bit_for_bit_and_follows_the_learning_rate(cont):
    """Three learns, eager vs warm-up + capture + replay: results, weights, Adam moments and the multiplier block are the same bits.  Then the
    cosine decay reaches lr = 0 (step = run_step): a replayed learn moves neither a weight nor a multiplier; after learning_rate_decay to a non-zero
    lr the same graph moves both."""
    from jorldy_amd.core.agent import Agent

    S, A, W, Tn, B = (5, 3, 4, 16, 24) if cont else (4, 2, 4, 16, 24)
    out = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        agent = Agent("vmpo", state_size=S, action_size=A, hidden_size=32, network="continuous_policy_value" if cont else "discrete_policy_value",
                      optim_config={"name": "adam", "lr": 1e-3}, batch_size=B, n_step=Tn, num_workers=W, run_step=4 * Tn, lr_decay=True, eta=2.0, alpha_mu=0.1, alpha_sigma=5.0,
                      device="cuda", use_graph=use_graph)
        agent.memory.first_store = False
        np.random.seed(3)
        res = []
        for it in range(3):
            r = agent.process(_synthetic(S, A, W * Tn, cont, 10 + it), (it + 1) * Tn)
            torch.cuda.synchronize()
            res.append([r[k] for k in sorted(r)])
        out.append((res, _state(agent)))
        if not use_graph:
            assert not agent._graphs
            continue
        assert agent._graphs, "learn() was captured"
        n_graphs = len(agent._graphs)
        # the fourth learn runs at the lr of step 3 Tn and leaves lr = 0 behind (cosine at step = run_step)
        agent.process(_synthetic(S, A, W * Tn, cont, 20), 4 * Tn)
        torch.cuda.synchronize()
        assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(0.0, abs=1e-12)
        before = _state(agent)
        agent.lr_decay = False
        agent.process(_synthetic(S, A, W * Tn, cont, 21), 5 * Tn)
        torch.cuda.synchronize()
        after = _state(agent)
        n = agent._net.n_params
        assert torch.equal(after[:n], before[:n]) and torch.equal(after[3 * n : 3 * n + 3], before[3 * n : 3 * n + 3]), "lr 0: weights and multipliers stay"
        assert not torch.equal(after[n : 3 * n], before[n : 3 * n]), "the moments still follow the gradients"
        agent.learning_rate_decay(2 * Tn)
        assert agent.optimizer.param_groups[0]["lr"] > 1e-4
        agent.process(_synthetic(S, A, W * Tn, cont, 22), 6 * Tn)
        torch.cuda.synchronize()
        moved = _state(agent)
        assert not torch.equal(moved[:n], after[:n]) and not torch.equal(moved[3 * n : 3 * n + 2], after[3 * n : 3 * n + 2]), "a non-zero lr reaches weights and multipliers"
        assert len(agent._graphs) == n_graphs, "no new capture: the replayed graph read the new learning rate"
    assert np.array_equal(np.asarray(out[0][0]), np.asarray(out[1][0])), "results: replay vs eager"
    assert torch.equal(out[0][1], out[1][1]), "weights, moments, multipliers: replay vs eager"


# ---------------------------------------------------------------------------------------------- checkpoints
def _small_agent(cont, **over):
    from jorldy_amd.core.agent import Agent

    kw = dict(state_size=5 if cont else 4, action_size=3 if cont else 2, hidden_size=32, network="continuous_policy_value" if cont else "discrete_policy_value",
              optim_config={"name": "adam", "lr": 1e-3}, batch_size=24, n_step=16, num_workers=4, run_step=10000, lr_decay=True, eta=2.0, alpha_mu=0.1, alpha_sigma=5.0,
              device="cuda")
    kw.update(over)
    agent = Agent("vmpo", **kw)
    agent.memory.first_store = False
    return agent


def _learn(agent, cont, it):
    r = agent.process(_synthetic(agent._net.S, agent._net.A, 64, cont, 30 + it), (it + 1) * 16)
    torch.cuda.synchronize()
    return [r[k] for k in sorted(r)]


@pytest.mark.parametrize("cont", [False, True])
def test_save_load_roundtrip_in_the_reference_format(cont, tmp_path):
    from tests.mirror.networks import Network

    torch.manual_seed(1)
    a = _small_agent(cont)
    np.random.seed(1)
    for it in range(2):
        _learn(a, cont, it)
    a.save(str(tmp_path))
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert set(ckpt) == {"network", "optimizer"} and list(ckpt["network"]) == list(a.network.state_dict())
    n_tensors = len(list(a.network.parameters()))
    # the multipliers that took steps carry moments; a discrete policy's alpha_sigma has no entry at all (torch's Adam skipped it)
    assert sorted(ckpt["optimizer"]["state"]) == list(range(n_tensors + (3 if cont else 2)))
    assert len(ckpt["optimizer"]["param_groups"][0]["params"]) == n_tensors + 3
    # the reference's optimizer on the CPU takes it: Adam over the network's parameters + three scalars
    m = Network("continuous_policy_value" if cont else "discrete_policy_value", a._net.S, a._net.A, D_hidden=32, head="mlp")
    scalars = [torch.nn.Parameter(torch.tensor(1.0)) for _ in range(3)]
    opt = torch.optim.Adam(list(m.parameters()) + scalars, lr=1e-3)
    opt.load_state_dict(ckpt["optimizer"])
    blk = a.multipliers()
    assert float(opt.state[scalars[0]]["exp_avg"]) == np.float32(blk["eta"]["m"]) and float(opt.state[scalars[0]]["step"]) == a._adam_steps == 6
    assert (scalars[2] in opt.state) == cont
    torch.manual_seed(2)
    b = _small_agent(cont)
    b.load(str(tmp_path))
    torch.cuda.synchronize()
    assert torch.equal(b._net.params, a._net.params) and torch.equal(b._net.m, a._net.m) and torch.equal(b._net.v, a._net.v) and b._adam_steps == a._adam_steps
    blk_b = b.multipliers()
    for j, n in enumerate(D.NAMES):
        assert blk_b[n]["value"] == np.float32((2.0, 0.1, 5.0)[j]), "the values are not in the reference's checkpoint: they stand at the constructor's"
        assert blk_b[n]["m"] == blk[n]["m"] and blk_b[n]["v"] == blk[n]["v"] and blk_b[n]["has_state"] == blk[n]["has_state"] == (cont or n != "alpha_sigma")


@pytest.mark.parametrize("cont", [False, True])
def test_save_full_load_full_resumes_bit_for_bit(cont, tmp_path):
    torch.manual_seed(1)
    a = _small_agent(cont)
    np.random.seed(1)
    for it in range(2):
        _learn(a, cont, it)
    a.save_full(str(tmp_path))
    saved = a._mult.clone()
    want = [_learn(a, cont, it) for it in (2, 3)]
    torch.manual_seed(5)
    np.random.seed(99)
    b = _small_agent(cont)
    b.load_full(str(tmp_path))
    assert npy(b._mult).tobytes() == npy(saved).tobytes() and b.time_t == 32 and b._adam_steps == 6
    got = [_learn(b, cont, it) for it in (2, 3)]
    assert np.array_equal(np.asarray(got), np.asarray(want)), "two further learns after load_full vs the uninterrupted agent"
    assert torch.equal(_state(b), _state(a))


# ---------------------------------------------------------------------------------------------- the reference's configurations
CONFIGS = [("cartpole", dict(state_size=4, action_size=2, network="discrete_policy_value", batch_size=64, n_step=128, _lambda=0.95, eps_eta=0.02, eps_alpha_mu=0.1,
                             eps_alpha_sigma=0.1, eta=2.0, alpha_mu=0.1, alpha_sigma=5.0, optim_config={"name": "adam", "lr": 2.5e-4}, num_workers=8)),
           ("mujoco", dict(state_size=11, action_size=3, network="continuous_policy_value", batch_size=64, n_step=128, _lambda=0.95, eps_eta=0.01, eps_alpha_mu=0.01,
                           eps_alpha_sigma=5e-5, eta=1.0, alpha_mu=1.0, alpha_sigma=1.0, optim_config={"name": "adam", "lr": 5e-4}, num_workers=4))]


@pytest.mark.parametrize("label,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_reference_config_constructs_and_learns_once(label, kw):
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    np.random.seed(0)
    agent = Agent("vmpo", gamma=0.99, n_epoch=1, min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, lr_decay=True, run_step=100000, device="cuda", **kw)
    assert agent._net.H == 512 and agent.batch_size == 64
    agent.memory.first_store = False
    cont = kw["network"].startswith("continuous")
    M = kw["num_workers"] * 128
    a = agent.act(np.zeros((kw["num_workers"], kw["state_size"]), np.float32))["action"]
    assert a.shape == (kw["num_workers"], kw["action_size"] if cont else 1)
    r = agent.process(_synthetic(kw["state_size"], kw["action_size"], M, cont, 1), 128)
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in r.values()), r
    assert agent._adam_steps == M // 64 and r["eta"] != kw["eta"] and (r["alpha_sigma"] != kw["alpha_sigma"]) == cont


def test_batch_size_and_single_row_minibatch_errors():
    from jorldy_amd.core.agent import Agent

    with pytest.raises(ValueError, match="batch_size <= 1024"):
        Agent("vmpo", state_size=4, action_size=2, batch_size=1025, device="cuda")
    agent = Agent("vmpo", state_size=4, action_size=2, hidden_size=32, batch_size=3, n_step=2, num_workers=2, device="cuda")
    agent.memory.first_store = False
    with pytest.raises(ValueError, match="NaN"):
        agent.process(_synthetic(4, 2, 4, False, 1), 2)
    with pytest.raises(NotImplementedError):
        agent._capture_targets(4)
    agent.grad_sync = object()
    with pytest.raises(NotImplementedError, match="data-parallel"):
        agent.learn()


# ---------------------------------------------------------------------------------------------- learning curve
def _hip_curve(seed):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    c = D.CURVE_CONFIG
    W, Tn = c["workers"], c["n_step"]
    np.random.seed(seed)
    torch.manual_seed(seed)
    agent = Agent("vmpo", run_step=c["run_step"], num_workers=W, device="cuda", seed=seed, **c["agent"])
    agent.memory.first_store = False
    env = ops.CartPoleVec(W, seed=1000 + seed)
    curve, step = [], 0
    S = np.empty((Tn, W, 4), np.float32)
    N = np.empty((Tn, W, 4), np.float32)
    Aa = np.empty((Tn, W, 1), np.float32)
    R = np.empty((Tn, W, 1), np.float32)
    Dn = np.empty((Tn, W, 1), np.float32)
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
    """config.vmpo.cartpole, 8 workers x 128 steps x 40 iterations on ops.CartPoleVec, seeds 1-3, against the curves of the UNMODIFIED reference
    agent on the oracle's CartPole (tests/golden/curves_reference_vmpo.json, tools/gen_golden_vmpo.py).  A curve is summarised as the mean of its
    last five iterations over its first iteration: both sides reach at least 3x, and the HIP end (mean episode length over the last five
    iterations, averaged over the seeds) lies within a factor 2 of the reference's -- the DQN CartPole test's criterion."""
    with open(os.path.join(ROOT, "tests", "golden", "curves_reference_vmpo.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_vmpo.py --only curves"
    ref = fx["vmpo_cartpole"]["reference"]
    hip = [_hip_curve(s) for s in D.CURVE_CONFIG["seeds"]]
    g_gain, r_gain = [D.curve_gain(c) for c in hip], [D.curve_gain(c) for c in ref]
    g_end, r_end = float(np.mean([np.mean(c[-5:]) for c in hip])), float(np.mean([np.mean(c[-5:]) for c in ref]))
    # the curves go beside the margin ledger (the scratch directory tests/margins.py writes to), before anything is asserted
    margins.record(max(g_end / r_end, r_end / g_end), 2.0, "vmpo: end of the HIP curves vs end of the reference's, as a factor")
    with open(os.path.join(os.path.dirname(margins.dump()), "learning_curve_vmpo_cartpole.json"), "w") as f:
        json.dump({"config": fx["config"], "metric": fx["metric"], "hip": hip, "reference": ref, "hip_gain": g_gain, "reference_gain": r_gain, "hip_end": g_end,
                   "reference_end": r_end}, f)
    print(f"V-MPO CartPole: HIP gains {g_gain}, end {g_end:.1f}; reference gains {r_gain}, end {r_end:.1f}")
    assert all(np.isfinite(c).all() for c in hip)
    assert min(g_gain) >= 3.0 and min(r_gain) >= 3.0, "both learn: the last five iterations over the first"
    assert 0.5 * r_end <= g_end <= 2.0 * r_end
