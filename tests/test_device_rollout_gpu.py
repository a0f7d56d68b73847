"""The device-resident rollout (csrc/jh_devroll.hip through manager.DeviceCollector) against the host envs, the float64 policy and the sampling
stream recomputed in numpy, at every shape at which the kernel can go wrong: one row, a row tile less / exactly / plus one row, three tiles,
more workgroups than the card has CUs; T = 1, 2 and 70 (several CartPole episodes end inside one launch); H = 16 (one column tile, one
k chunk: three of the four waves idle), 64, 512 (more than 64 KB of LDS) and the cap 1024; the control env at (S 11, A 3) and at its caps (S 64, A 16: three head tiles)."""
import functools

import numpy as np
import pytest
import torch

import acting_truth as AT
import fp64_truth as F
from util import npy

pytestmark = pytest.mark.gpu

U = np.uint64
C1, FNV = U(0x9E3779B97F4A7C15), U(0x100000001B3)
BIG = "more workgroups than CUs"
#        kind  W    T   H    S   A
CASES = [("cp", 1, 1, 16, 4, 2), ("cp", 15, 2, 64, 4, 2), ("cp", 16, 70, 512, 4, 2), ("cp", 17, 70, 64, 4, 2), ("cp", 33, 70, 64, 4, 2), ("cp", BIG, 2, 64, 4, 2),
         ("ct", 1, 1, 16, 11, 3), ("ct", 17, 70, 64, 11, 3), ("ct", 33, 70, 64, 11, 3), ("ct", 16, 2, 512, 64, 16), ("ct", 15, 70, 16, 64, 16),
         ("ct", 17, 2, 1024, 64, 16)]  # the cap, at the shapes that need the most LDS (152 KB)
ids = lambda c: "-".join(str(x).replace(" ", "_") for x in c)


def u01(key):
    return (AT._mix(key) >> U(11)).astype(np.float64) / 9007199254740992.0


def make(kind, W, T, H, S, A, env_seed=5, **kw):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import DeviceCollector

    if W == BIG:
        W = 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 1)
    case = {"S": S, "A": A, "H": H, "cont": kind == "ct", "W": W, "T": T}
    torch.manual_seed(11)
    agent = Agent("ppo", state_size=S, action_size=A, hidden_size=H, network=AT.network_name(case), n_step=T, batch_size=32, n_epoch=2, device="cuda", seed=3,
                  lr_decay=False, num_workers=W, **kw)
    with torch.no_grad():
        for p in agent.network.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))  # every bias off zero
    agent.memory.first_store = False
    env = ops.DeviceCartPole(W, env_seed, "cuda") if kind == "cp" else ops.DeviceControl(W, S, A, env_seed, "cuda")
    return case, agent, env, DeviceCollector(env, agent, W)


def read(case, agent):
    W, T, M = case["W"], case["T"], case["W"] * case["T"]
    out = {k: npy(agent.memory._store.column(k)[:M]).copy().reshape((W, T) + ((-1,) if k in ("state", "next_state", "action") else ())) for k in
           ("state", "action", "reward", "next_state", "done")}
    if agent._captured:
        out.update({k: npy(agent._static[k]).copy().reshape(W, T, -1) for k in ("h0", "h1", "value", "next_value") if agent._static[k] is not None})
    return out


@functools.lru_cache(maxsize=None)
def rollout(c, training=True, env_seed=5, again=0):
    """One run of the case from fresh seeds -> (case, weights, (seed, counter before), counter after, rows + capture, env rng words before).
    `again` only makes another cache entry: the same configuration run afresh."""
    case, agent, env, col = make(*c, env_seed=env_seed)
    sd = {k: v.detach().cpu().clone() for k, v in agent.network.state_dict().items()}
    rng0, before = env.state()["rng"], agent._net.act_rng()
    assert np.array_equal(env.obs(), host_env(case, env_seed).obs()), "a device env starts as the host env of its seed"
    col.run(case["T"], training=training)
    torch.cuda.synchronize()
    return case, sd, before, agent._net.act_rng()[1], read(case, agent), rng0


def host_env(case, seed=5):
    from jorldy_amd import ops

    return ops.ControlVec(case["W"], case["S"], case["A"], seed) if case["cont"] else ops.CartPoleVec(case["W"], seed)


def heads_are_the_policys(case, sd, r, what):
    m64, m32 = AT.modules_of(case, sd)
    truth = AT.truths(case, m64, m32, r["state"], r["next_state"])
    go = torch.from_numpy(~r["done"].reshape(-1).astype(bool))
    for q, (exact, ref32) in truth.items():
        ours = torch.from_numpy(r[q]).reshape(exact.shape)
        if q == "next_value":  # where done, ours is V(reset state): covered by next_value[w, t] == value[w, t + 1] below
            ours, exact, ref32 = ours[go], exact[go], ref32[go]
        F.vs_exact(ours, exact, ref32, 1e-5, f"{what} captured {q}")
    assert np.array_equal(r["next_value"][:, :-1], r["value"][:, 1:])


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_env_is_the_host_env_on_the_stored_actions(c):
    case, _, _, _, r, _ = rollout(c)
    W, T = case["W"], case["T"]
    env = host_env(case)
    done = r["done"].astype(bool)
    for t in range(T):
        obs = env.obs()
        nxt, rew, dn = env.step(r["action"][:, t] if case["cont"] else r["action"][:, t, 0])
        assert np.array_equal(dn.astype(bool), done[:, t]) and np.array_equal(rew, r["reward"][:, t]), t
        for ours, host in ((r["state"][:, t], obs), (r["next_state"][:, t], nxt)):
            assert np.all(np.abs(ours - host) <= np.spacing(np.abs(host))), t
        if t + 1 < T:
            cont = ~done[:, t]
            assert np.array_equal(r["state"][cont, t + 1], r["next_state"][cont, t])
            assert np.array_equal(r["state"][done[:, t], t + 1], env.obs()[done[:, t]]), "the reset observation is the host's, bit for bit"
    if T == 70 and not case["cont"]:
        assert (done.sum(1) >= 2).any(), "several episodes end inside one launch"


def test_cartpole_ends_at_500_steps():
    case, agent, env, col = make("cp", 17, 4, 64, 4, 2)
    st = env.state()
    rows = np.array([3, 16])
    st["t"][rows] = 497
    env.set_state(t=st["t"])
    col.run(4)
    r = read(case, agent)
    late = np.zeros(17, bool)
    late[rows] = True
    assert np.array_equal(r["done"] == 1, late[:, None] & (np.arange(4) == 2)[None, :])
    assert np.all(r["reward"][late, 2] == -1.0) and np.all(r["reward"][~late] == np.float32(0.1))
    with np.errstate(over="ignore"):
        fresh = -0.05 + 0.1 * u01(st["rng"][rows, None] + np.arange(4, dtype=U)[None, :] * C1)
    assert np.array_equal(r["state"][late, 3], fresh.astype(np.float32))
    assert np.array_equal(env.state()["t"], np.where(late, 1, 4))


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_captured_heads_and_values_are_the_float64_policys(c):
    case, sd, _, _, r, _ = rollout(c)
    heads_are_the_policys(case, sd, r, ids(c))


def check_actions(case, r, seed, ctr, training):
    """-> rows left out (discrete: u within 1e-5 of a CDF boundary of the float64 softmax of the captured logits)."""
    W, T, A = case["W"], case["T"], case["A"]
    w, t = np.arange(W, dtype=U)[:, None], np.arange(T, dtype=U)[None, :]
    with np.errstate(over="ignore"):
        base = U(seed) * FNV + (U(ctr) + t) * C1
        if not case["cont"]:
            z = r["h0"].astype(np.float64)
            if not training:
                top = np.sort(z, -1)
                sure = top[..., -1] - top[..., -2] > 1e-4
                assert np.array_equal(r["action"][..., 0][sure], z.argmax(-1)[sure])
                return 0
            p = np.exp(z - z.max(-1, keepdims=True))
            cdf = np.cumsum(p / p.sum(-1, keepdims=True), -1)[..., :-1]
            u = u01(base + w)[..., None]
            sure = np.abs(u - cdf).min(-1) > 1e-5
            assert np.array_equal(r["action"][..., 0][sure], (u >= cdf).sum(-1)[sure])
            return int((~sure).sum())
        mu = np.clip(r["h0"].astype(np.float64), -5, 5)
        if training:
            key = (base + w * U(64))[..., None] + np.arange(A, dtype=U)
            u1, u2 = 1.0 - u01(key * U(2) + U(1)), u01(key * U(2) + U(2))
            mu = mu + np.exp(np.tanh(r["h1"].astype(np.float64))) * np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)
        assert np.abs(r["action"] - np.tanh(mu)).max() <= 1e-5
        return 0


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_stored_actions_are_the_streams_draws(c):
    case, _, (seed, ctr), ctr_after, r, _ = rollout(c)
    assert ctr_after == ctr + case["T"]
    assert check_actions(case, r, seed, ctr, True) == 0, "these seeds put no u within 1e-5 of a CDF boundary"


@pytest.mark.parametrize("c", [CASES[3], CASES[7]], ids=ids)
def test_greedy_actions(c):
    case, _, (seed, ctr), ctr_after, r, _ = rollout(c, training=False)
    assert ctr_after == ctr + case["T"]
    check_actions(case, r, seed, ctr, False)


@pytest.mark.parametrize("small, wide", [(CASES[3], CASES[4]), (CASES[7], CASES[8])], ids=["cp", "ct"])
def test_a_rows_output_does_not_depend_on_the_tiling(small, wide):
    a, b = rollout(small)[4], rollout(wide)[4]
    again = rollout(small, again=1)[4]
    for k in a:
        assert np.array_equal(a[k], b[k][:17]), k
        assert np.array_equal(a[k], again[k]), k


@pytest.mark.parametrize("kind, S, A", [("cp", 4, 2), ("ct", 11, 3)])
def test_rows_feed_learn(kind, S, A, monkeypatch):
    W, T = 17, 8
    monkeypatch.setenv("JH_COLLECT_CAPTURE", "0")
    (case, dev, _, col), (_, twin, _, _) = make(kind, W, T, 64, S, A), make(kind, W, T, 64, S, A)
    col.run(T)
    rows = read(case, dev)
    assert dev._captured == 0
    results = []
    for agent, given in ((dev, None), (twin, {k: v.reshape(W * T, -1) for k, v in rows.items()})):
        np.random.seed(7)
        results.append(agent.process(given, T))
        torch.cuda.synchronize()
    assert results[0] and results[0] == results[1]
    for b in ("params", "m", "v"):
        assert torch.equal(getattr(dev._net, b), getattr(twin._net, b)), b
    monkeypatch.setenv("JH_COLLECT_CAPTURE", "1")
    case, agent, env, col = make(kind, W, T, 64, S, A)
    col.run(T)
    res = agent.process(None, T)
    assert all(np.isfinite(v) for v in res.values()) and agent.memory.size == 0
    sd = {k: v.detach().cpu().clone() for k, v in agent.network.state_dict().items()}
    col.run(T)
    torch.cuda.synchronize()
    heads_are_the_policys(case, sd, read(case, agent), f"{kind} second run")


def test_refusals_name_what_is_eligible():
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import DeviceCollector

    cp, ct = ops.DeviceCartPole(4, 0, "cuda"), ops.DeviceControl(4, 4, 2, 0, "cuda")
    ppo = lambda **kw: Agent("ppo", **{**dict(state_size=4, action_size=2, hidden_size=64, device="cuda"), **kw})
    for env, agent in ((cp, Agent("vmpo", state_size=4, action_size=2, hidden_size=64, device="cuda")),
                       (cp, ppo(state_size=[4, 84, 84], head="cnn")), (ct, ppo()), (cp, ppo(hidden_size=1040))):
        with pytest.raises(ValueError, match="DeviceCollector runs the PPO agent on the MLP head only"):
            DeviceCollector(env, agent)
