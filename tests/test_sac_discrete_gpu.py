"""The discrete SAC on the GPU: both kernels of csrc/jh_sac_discrete.hip against the float64 truth of tests/sacd_truth.py (pinned to the reference's
own learn() by tests/test_sac_discrete_cpu.py) at every lane-group width and workgroup edge, bit-identical runs and graph replays, then the agent
against the fixtures of tools/gen_golden_sac_discrete.py, its checkpoints, the configs' shapes and the CartPole curve next to the reference's."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import margins
import sacd_truth as D
from tests.util import f32, load, npy

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))  # the fixtures' keyword sets, the curve loop
STEPS = {"static": None, "dyn0": 0, "dyn1": 1}
BUF_KEYS = ("state", "action", "reward", "next_state", "done")
ONLINE = ("actor", "critic1", "critic2")


def _blocks(c, ops):
    k = STEPS[c["mode"]]
    blk = ops.sacd_temperature(D.LOG_ALPHA, -np.log(1 / c["A"]) * 0.98, alpha=D.ALPHA, m=D.PRIOR_M if k else 0.0, v=D.PRIOR_V if k else 0.0, has_state=bool(k))
    return blk, ops.vmpo_hyper(D.ALPHA_LR, step=k or 0), k


def _run(c, ops, x, work, blk, hyper, k, stats, out=(None, None, None)):
    g1, g2, _ = ops.sacd_critic_loss(x["la_next"], x["qt1"], x["qt2"], x["q1"], x["q2"], x["action"], x["reward"], x["done"], D.GAMMA, blk, stats=stats, work=work, out=out[:2])
    g_la, _ = ops.sacd_actor_loss(x["la"], x["q1_pi"], x["q2_pi"], blk, hyper, k is not None, stats=stats, work=work, out=out[2])
    return g1, g2, g_la, stats, blk, hyper


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_kernels_match_float64(c):
    """Every output of both kernels within twice the case's recorded float32 gap (sacd_truth.distance), the rule of tests/test_r2d2_actors_edges_gpu.py."""
    from jorldy_amd import ops

    x = {k: f32(v) for k, v in D.case_inputs(c).items()}
    g1, g2, g_la, stats, blk, hyper = _run(c, ops, x, ops.sacd_workspace(), *_blocks(c, ops), torch.full((8,), -1.0, device="cuda"))
    want, k = D.case_truth(c)[:2]
    s, b = npy(stats).astype(np.float64), ops.vmpo_block_read(blk)
    got = dict({"dQ1": npy(g1), "dQ2": npy(g2), "d logits": npy(g_la), "log_alpha": b["eta"]["value"]}, **{n: s[i] for i, n in enumerate(ops.SACD_STATS)})
    assert set(got) == set(want)
    err, where = D.distance(got, want)
    print(f"{D.case_id(c)}: worst {err:.3e} at {where}, allowed {2 * c['gap']:.3e}")
    margins.leq(err, 2 * c["gap"], f"{D.case_id(c)} {where} vs float64")
    if c.get("near"):  # the row's terms are formed in double and rounded once: every ENTRY within a float32 ulp; keeping the derivative under the clamp moves the small lanes' by 6 %
        margins.leq(float(np.abs(got["d logits"] / want["d logits"] - 1).max()), 2.0 ** -23, f"{D.case_id(c)} d logits, entrywise")
    assert b["alpha_mu"]["value"] == s[6] == np.float32(np.exp(np.float64(np.float32(D.LOG_ALPHA)))), "the alpha in use is refreshed from log_alpha before its step"
    assert int(npy(hyper)[4]) == (0 if k is None else k + 1) and b["eta"]["has_state"] == (k is not None), "the temperature's own step count"
    assert k is not None or (b["eta"]["value"] == np.float32(D.LOG_ALPHA) and b["eta"]["m"] == 0 and b["eta"]["v"] == 0), "a static temperature moved"


def test_runs_and_graph_replays_are_bit_identical():
    from jorldy_amd import ops

    flat = lambda o: torch.cat([t.reshape(-1) for t in o]).clone()
    for c in (c for c in D.CASES if (c["A"], c["B"]) in ((3, 65), (5, 1024), (64, 1024))):  # two workgroups at A 3; 32 and 256 workgroups at B 1024
        x = {k: f32(v) for k, v in D.case_inputs(c).items()}
        work = ops.sacd_workspace()
        eager = [flat(_run(c, ops, x, work, *_blocks(c, ops), torch.zeros(8, device="cuda"))) for _ in range(2)]
        assert torch.equal(eager[0], eager[1]), "a second run on the same workspace"
        blk, hyper, k = _blocks(c, ops)
        blk0, hyper0, stats = blk.clone(), hyper.clone(), torch.zeros(8, device="cuda")
        outs = (torch.empty_like(x["q1"]), torch.empty_like(x["q1"]), torch.empty_like(x["la"]))
        body = lambda: _run(c, ops, x, work, blk, hyper, k, stats, outs)
        body()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with ops.graph_capture(g):
            body()
        for _ in range(3):
            blk.copy_(blk0)
            hyper.copy_(hyper0)
            g.replay()
            assert torch.equal(flat(outs + (stats, blk, hyper)), eager[0]), f"{D.case_id(c)}: a replay differs from the eager run"


# ----------------------------------------------------------------------------------------------- the agent
def _fixture_agent(name, z, **over):
    import gen_golden_sac_discrete as G
    from jorldy_amd.core.agent import Agent
    from oracle import synth

    h = lambda k: z[f"hyper/{k}"].item()
    kw = {**G.agent_kwargs(G.SPECS[name]), "device": "cuda", "lr_decay": False, "target_update_period": 10 ** 9, **over}
    torch.manual_seed(int(h("init_seed")))
    agent = Agent("sac", **kw)
    for i, net in enumerate(D.NETS):  # the initial weights: the reference's construction order and initialisers under the same seed
        view = getattr(agent, net)
        sd = view.state_dict()
        for k, v in sd.items():
            ref = z[f"init_thin/{net}/{k}"]  # orthogonal_init's QR differs between hosts by its H-term sums' roundings: tests/test_r2d2_gpu.py's bound
            margins.leq(float(np.abs(synth.thin(npy(v)) - ref).max()), kw["hidden_size"] * 2.0 ** -23 * float(np.abs(ref).max()) + 1e-30, f"initial {net} {k}")
        view.load_state_dict(synth.recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, int(h("recipe_seed")) + i) if int(h("recipe")) else {k: z[f"sd0/{net}/{k}"] for k in sd})
    agent.memory.first_store = False
    agent.memory.store([{k: z[f"buf_{k}"][i : i + 1] for k in BUF_KEYS} for i in range(len(z["buf_state"]))])
    return agent


@pytest.mark.parametrize("name", D.FIXTURES)
def test_agent_learn_matches_the_reference_records(name):
    """Record by record from the recorded state and numpy seed: the result keys and the tapped tensors within 1e-5, then gradients (1e-5 of the
    tensor's largest entry), Adam moments (2e-5) and weights (at most 0.5 % further than 2e-5, the worst within 2.1 lr): the tolerances of
    tests/test_sac_gpu.py.  Weights and moments are teacher-forced between records, the temperature is left as the device advanced it: the
    third record of sac_discrete.npz fails if alpha does not lag by one learn.  sac_discrete_static.npz: the hard update between its learns."""
    from oracle import synth

    z = load(name)
    agent = _fixture_agent(name, z)
    limit, dynamic, nets = int(z["hyper/thin_limit"]), bool(int(z["hyper/use_dynamic_alpha"])), agent._nets
    thin = (lambda a: synth.thin(a, limit)) if limit else (lambda a: a)
    for i in range(int(z["hyper/records"])):
        r, p = f"r{i}", f"r{i - 1}"
        for net in ONLINE if i > 0 else ():
            for bucket, pre in ((None, f"{p}/sd1/{net}/"), (nets[net].m, f"{p}/opt/{net}/exp_avg/"), (nets[net].v, f"{p}/opt/{net}/exp_avg_sq/")):
                nets[net].import_state({k: z[pre + k] for k in nets[net].export_state()}, bucket)
        if f"{r}/target0/target_critic1/l.weight" in z.files:
            before = nets["critic1"].target.clone()
            agent.update_target_hard()
            assert not torch.equal(before, nets["critic1"].target)
            for t in ("target_critic1", "target_critic2"):
                assert all(np.array_equal(npy(v), z[f"{r}/target0/{t}/{k}"]) for k, v in getattr(agent, t).state_dict().items()), f"{r} {t} after the hard update"
        t0 = agent.temperature()
        np.testing.assert_allclose(t0["alpha"], z[f"{r}/alpha0/alpha"], rtol=2e-7, err_msg=f"{r}: the alpha in use")
        np.testing.assert_allclose(t0["log_alpha"], z[f"{r}/alpha0/log_alpha"], rtol=1e-5, err_msg=f"{r} log_alpha before")
        targets = [nets[c].target.clone() for c in ONLINE[1:]]
        np.random.seed(int(z[f"{r}/np_seed"]))
        result = agent.learn()
        assert all(torch.equal(nets[c].target, t) for c, t in zip(ONLINE[1:], targets)), "learn() moved a target"
        assert set(result) == {k.split("/")[-1] for k in z.files if k.startswith(f"{r}/result/")}
        for k, v in result.items():
            np.testing.assert_allclose(v, z[f"{r}/result/{k}"], rtol=1e-5, atol=1e-7, err_msg=f"{r} {k}")
        st = agent._static
        assert np.array_equal(npy(st["tr"]["state"]), z[f"{r}/learn/state"]), "other rows were sampled"
        for ours, key in ((st["la"][1], "logits_next"), (st["la"][0], "logits"), (st["lq"][0][0], "q1_all"), (st["lq"][1][0], "q2_all"), (st["lq"][0][2], "qt1_next"), (st["lq"][1][2], "qt2_next"),
                          (st["q_pi"][0], "q1_after"), (st["q_pi"][1], "q2_after"), (st["g_q"][0], "d_q1_all"), (st["g_q"][1], "d_q2_all"), (st["g_la"], "d_logits")):
            np.testing.assert_allclose(npy(ours).reshape(-1), z[f"{r}/learn/{key}"].reshape(-1), rtol=1e-5, atol=1e-5, err_msg=f"{r} {key}")
        tot, bad, worst = 0, 0, 0.0
        for net in ONLINE:
            for bucket, pre, tol in ((nets[net].grads, f"{r}/grad/{net}/", 1e-5), (nets[net].m, f"{r}/opt/{net}/exp_avg/", 2e-5), (nets[net].v, f"{r}/opt/{net}/exp_avg_sq/", 2e-5)):
                for k, v in nets[net].export_state(bucket).items():
                    scale = float(z[f"{r}/grad_absmax/{net}/{k}"]) if "grad" in pre else float(np.abs(z[pre + k]).max())
                    margins.leq(float(np.abs(thin(npy(v)).astype(np.float64) - z[pre + k]).max()) / (scale + 1e-30), tol, f"{pre}{k}: max |diff| / the tensor's largest entry")
            for k, v in nets[net].export_state().items():
                dd = np.abs(thin(npy(v)) - z[f"{r}/sd1/{net}/{k}"])
                tot, bad, worst = tot + dd.size, bad + int((dd > 2e-5).sum()), max(worst, float(dd.max()) / float(z["hyper/actor_lr" if net == "actor" else "hyper/critic_lr"]))
        margins.leq(bad / tot, 0.005, f"{r} fraction of weights further than 2e-5 from the reference's")
        margins.leq(worst, 2.1, f"{r} worst weight difference / lr vs the possible travel")
        t1 = agent.temperature()
        assert t1["alpha"] == result["alpha"] and t1["step"] == int(z[f"{r}/alpha1/step"])
        if dynamic:
            w, w0 = float(z[f"{r}/alpha1/log_alpha"]), float(z[f"{r}/alpha0/log_alpha"])
            margins.leq(abs(t1["log_alpha"] - w), 2.0 ** -22 * abs(w) + 1e-4 * abs(w - w0) + 1e-6 * float(z["hyper/alpha_lr"]), f"{r} log_alpha after its step")
            np.testing.assert_allclose([t1["m"], t1["v"]], [z[f"{r}/alpha1/exp_avg"], z[f"{r}/alpha1/exp_avg_sq"]], rtol=2e-5, err_msg=f"{r} alpha moments")
        else:
            assert t1["log_alpha"] == t0["log_alpha"] == np.float32(z["hyper/static_log_alpha"]) and t1["alpha"] == t0["alpha"]


def _state_bits(agent):  # (the actor's target bucket is idle: not part of the agent's state)
    return torch.cat([b for k, n in agent._nets.items() for b in (n.params, n.m, n.v) + ((n.target,) if k != "actor" else ())] + [agent._temp, agent._temp_hyper]).clone()


def test_checkpoints_round_trip_and_resume_bit_for_bit(tmp_path):
    z = load("sac_discrete")
    a, b, c = (_fixture_agent("sac_discrete", z, target_update_period=2) for _ in range(3))
    buf = [{k: z[f"buf_{k}"][i : i + 1] for k in BUF_KEYS} for i in range(8)]
    np.random.seed(3)
    for it in range(3):
        a.process([buf[it]], it + 1)
    a.save(str(tmp_path))
    ck = torch.load(os.path.join(str(tmp_path), "ckpt"), map_location="cpu", weights_only=False)
    assert list(ck) == ["actor", "actor_optimizer", "critic1", "critic2", "critic_optimizer1", "critic_optimizer2", "log_alpha", "alpha_optimizer"]
    for net, okey in zip(ONLINE + ("log_alpha",), ("actor_optimizer", "critic_optimizer1", "critic_optimizer2", "alpha_optimizer")):  # loadable by torch's own classes
        params = [torch.nn.Parameter(v.clone()) for v in (ck[net].values() if net in ONLINE else [ck[net].detach()])]
        opt = torch.optim.Adam(params)
        opt.load_state_dict(ck[okey])
        last = list(a._nets[net].export_state(a._nets[net].m).values())[-1].cpu() if net in ONLINE else torch.tensor([a.temperature()["m"]])
        assert int(opt.state[params[0]]["step"]) == 3 and torch.equal(opt.state[params[-1]]["exp_avg"].cpu(), last)
    b.load(str(tmp_path))
    assert torch.equal(b._nets["critic2"].params, a._nets["critic2"].params) and torch.equal(b._nets["critic2"].target, a._nets["critic2"].params)
    assert b.log_alpha == a.log_alpha == float(ck["log_alpha"]) and b.temperature()["step"] == 3 and b.alpha == float(np.exp(np.float32(a.log_alpha)))
    b.sync_in(a.sync_out()["weights"])
    assert torch.equal(b._nets["actor"].params, a._nets["actor"].params)
    # the complete checkpoint: the resumed agent continues bit for bit, the stamp and the temperature's lag included
    a.save_full(str(tmp_path))
    c.load_full(str(tmp_path))
    assert torch.equal(_state_bits(c), _state_bits(a)) and c.target_update_stamp == a.target_update_stamp
    rs = np.random.get_state()  # what load_full restored: both agents sample their batches from it
    ra = [a.process([buf[it]], it + 1) for it in range(3, 7)]
    np.random.set_state(rs)
    rc = [c.process([buf[it]], it + 1) for it in range(3, 7)]
    assert ra == rc and torch.equal(_state_bits(c), _state_bits(a))


CONFIGS = [("config.sac.cartpole_discrete", dict(state_size=4, action_size=2, batch_size=64, start_train_step=5000, static_log_alpha=-2.0, target_update_period=500)),
           ("config.sac.pong_mlagent", dict(state_size=8, action_size=3, batch_size=32, start_train_step=25000, static_log_alpha=-3.0, target_update_period=1000))]


@pytest.mark.parametrize("label,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_reference_config_constructs_acts_and_learns(label, kw):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent

    torch.manual_seed(0)
    kw = dict(kw, actor="discrete_policy", critic="discrete_q_network")
    agent = Agent("sac", device="cuda", use_dynamic_alpha=True, gamma=0.99, tau=5e-3, buffer_size=50000,
                  optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 1.5e-4, "critic_lr": 3e-4, "alpha_lr": 1e-5}, **kw)
    A, S = kw["action_size"], kw["state_size"]
    assert agent.action_type == "discrete" and agent.hidden_size == 512 and agent.log_alpha == 0.0 and agent.alpha == 1.0
    assert agent.target_entropy == -np.log(1 / A) * 0.98 and agent.temperature()["lr"] == np.float32(1e-5)
    rng = np.random.RandomState(0)
    for training in (True, False):
        a = agent.act(rng.randn(2, S).astype(np.float32), training)["action"]
        assert a.shape == (2, 1) and a.dtype == np.int64 and a.min() >= 0 and a.max() < A
    agent.memory.first_store = False
    agent.memory.store([{"state": rng.randn(1, S).astype(np.float32), "action": rng.randint(0, A, (1, 1)), "reward": rng.randn(1, 1), "next_state": rng.randn(1, S).astype(np.float32),
                         "done": rng.rand(1, 1) < 0.1} for _ in range(kw["batch_size"] + 1)])
    for _ in range(3):  # eager, capture + replay, replay
        res = agent.learn()
    assert set(res) == set(ops.SACD_STATS) and all(np.isfinite(v) for v in res.values()) and agent._graph is not None and agent.temperature()["step"] == 3
    for bad in (dict(head="cnn"), dict(action_size=65), dict(action_size=1), dict(batch_size=1025), dict(hidden_size=30), dict(critic="continuous_q_network"),
                dict(actor="continuous_policy"), dict(grad_sync=object()), dict(buffer_size=kw["batch_size"]), dict(device="cpu")):
        with pytest.raises(ValueError, match="libjorldy_hip"):
            Agent("sac", **{**kw, "device": "cuda", **bad})


_tenths = lambda c: (float(np.mean(c[: max(1, len(c) // 10)])), float(np.mean(c[-max(1, len(c) // 10) :])))  # first and last tenth of a curve


def test_cartpole_learning_curve_tracks_the_real_reference():
    """The JSON's configuration in single mode on ops.CartPoleVec (tools/bench_sac.py's discrete_curve) against the three curves of the UNMODIFIED
    reference on the oracle's CartPole (tools/gen_golden_sac_discrete.py): the mean of three seeds learns (last tenth above first tenth) and its end
    lies inside the band of the reference's own three seeds, widened by that file's own seed-to-seed spread (highest end / lowest end)."""
    import bench_sac

    with open(os.path.join(os.path.dirname(__file__), "golden", "curves_reference_sac_discrete.json")) as f:
        fx = json.load(f)
    r_first, r_last = zip(*(_tenths(c) for c in fx["sac_discrete"]["reference"]))
    assert fx["seeds"] == [1, 2, 3] and np.mean(r_last) > np.mean(r_first), "the reference itself learns at this budget"
    hip = [bench_sac.discrete_curve(s, fx["config"]) for s in fx["seeds"]]
    first, last = (float(np.mean(v)) for v in zip(*(_tenths(c) for c in hip)))
    spread = max(r_last) / min(r_last)
    print(f"HIP first / last tenth (mean of three seeds) {first:.1f} / {last:.1f}; reference ends {r_last}, spread {spread:.2f}; HIP curves {hip}")
    assert np.isfinite(hip).all() and last > first, "the curve learns"
    margins.leq(max(last / max(r_last), min(r_last) / last), spread, "end of the HIP curves vs the band of the reference's three seeds, as a factor")
