"""TD3's and SAC's device-resident actors (csrc/jh_devroll_ac.hip through manager.DeviceCollector) against the host control env, the float64
actor and the exploration stream recomputed in numpy, at the smallest shapes at which the kernel can go wrong: one row, a row tile less /
plus one row, three tiles, more workgroups than CUs; T = 1, 2 and 70; H = 16 (one column tile, one k chunk: three waves idle), 64, 512 (more
than 64 KB of LDS) and the cap; (S 11, A 3) and the env's caps (S 64, A 16: SAC's two output column tiles).  In the T = 70 cases the rows LATE
start at step count 997 (the host env cannot be put there: they are held to it up to their reset, and to the reset stream at it)."""
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
SEED, ENV_SEED, BIG, LATE = 9, 5, "more workgroups than CUs", [3, 16]
#        agent  W   T   H    S   A
CASES = [("td3", 1, 1, 16, 11, 3), ("td3", 15, 2, 64, 11, 3), ("td3", 17, 70, 64, 11, 3), ("sac", 17, 70, 64, 11, 3), ("sac", 33, 70, 64, 11, 3),
         ("sac", 16, 2, 512, 64, 16), ("td3", 17, 2, "cap", 64, 16), ("sac", 17, 2, "cap", 64, 16), ("sac", BIG, 2, 64, 11, 3)]
ids = lambda c: "-".join(str(x).replace(" ", "_") for x in c)


def u01(key):
    return (AT._mix(key) >> U(11)).astype(np.float64) / 9007199254740992.0


def make(name, W, T, H, S, A, env_cls="DeviceControl", **kw):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import DeviceCollector

    W = 16 * (torch.cuda.get_device_properties(0).multi_processor_count + 1) if W == BIG else W
    H = ops.DEVROLL_AC_MAX_H if H == "cap" else H
    torch.manual_seed(11)
    agent = Agent(name, **{**dict(state_size=S, action_size=A, hidden_size=H, batch_size=32, buffer_size=max(4096, W * T), start_train_step=0, lr_decay=False,
                                  device="cuda"), **kw})
    if type(agent).__name__ != "SACDiscrete":
        agent.actor.load_state_dict({k: v + 0.05 * torch.randn_like(v) if v.dim() == 1 else v for k, v in agent.actor.state_dict().items()})  # every bias off zero
    env = ops.DeviceCartPole(W, ENV_SEED, "cuda") if env_cls == "DeviceCartPole" else ops.DeviceControl(W, S, A, ENV_SEED, "cuda")
    return agent, env, DeviceCollector(env, agent, seed=SEED)


def run(col, T, training=True):
    col.capture_heads = True
    col.run(T, training=training)
    torch.cuda.synchronize()
    return {k: npy(v[: col.env.W * T]).copy().reshape(T, col.env.W, -1) for k, v in col._out.items()}


@functools.lru_cache(maxsize=None)
def rollout(c, training=True, again=0):
    """One run from fresh seeds -> (agent, collector, float64 actor weights, rows [T, W, ...], env rng words before); `again`: another cache entry."""
    agent, env, col = make(*c)
    st = env.state()
    if c[2] == 70:
        st["t"][LATE] = 997
        env.set_state(t=st["t"])
    sd = {k: v.detach().cpu().double() for k, v in agent.actor.state_dict().items()}
    return agent, col, sd, run(col, c[2], training), st["rng"]


def draws(W, T, A, ctr=0):
    """-> (u2, n) [T, W, A]: the second uniform and the standard normal of (SEED, ctr + t, row, k)."""
    t, w, k = np.arange(T, dtype=U)[:, None, None], np.arange(W, dtype=U)[None, :, None], np.arange(A, dtype=U)[None, None, :]
    with np.errstate(over="ignore"):
        key = U(SEED) * FNV + (U(ctr) + t) * C1 + w * U(64) + k
        u1, u2 = 1.0 - u01(key * U(2) + U(1)), u01(key * U(2) + U(2))
    return u2, np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)


def expected_actions(name, z, n, training, std=0.1):
    A = n.shape[-1]
    if name == "td3":
        return np.clip(np.tanh(z) + std * n, -1, 1) if training else np.tanh(z)
    mu = np.clip(z[..., :A], -5, 5)
    return np.tanh(mu + np.exp(np.tanh(z[..., A:])) * n if training else mu)


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_env_is_the_host_env_on_the_stored_actions(c):
    from jorldy_amd import ops

    _, col, _, r, rng0 = rollout(c)
    (T, W, S), A = r["state"].shape, c[5]
    env = ops.ControlVec(W, S, A, ENV_SEED)
    done, late = r["done"][..., 0].astype(bool), np.zeros(W, bool)
    if T == 70:
        late[LATE] = True
    for t in range(T):
        m = ~late | (t <= 2)  # the rows the host env still follows
        obs = env.obs()
        nxt, rew, dn = env.step(r["action"][t])
        assert np.array_equal(dn.astype(bool)[m] | (late[m] & (t == 2)), done[t, m]) and np.array_equal(rew[m], r["reward"][t, m, 0]), t
        for ours, host in ((r["state"][t], obs), (r["next_state"][t], nxt)):
            assert np.all(np.abs(ours - host)[m] <= np.spacing(np.abs(host))[m]), t
        if t + 1 < T:
            assert np.array_equal(r["state"][t + 1][~done[t]], r["next_state"][t][~done[t]])
            assert np.array_equal(r["state"][t + 1][done[t] & ~late], env.obs()[done[t] & ~late]), "the reset observation is the host's, bit for bit"
    if T == 70:
        with np.errstate(over="ignore"):
            fresh = -0.05 + 0.1 * u01(rng0[LATE, None] + np.arange(S, dtype=U)[None, :] * C1)
        assert done[2, LATE].all() and done.sum() == len(LATE), "episodes end inside the launch: the rows that started at step 997"
        assert np.array_equal(r["state"][3, LATE], fresh.astype(np.float32)) and np.array_equal(col.env.state()["t"], np.where(late, 67, 70))


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_heads_are_the_float64_actors(c):
    _, _, sd, r, _ = rollout(c)
    last = ("pi",) if c[0] == "td3" else ("mu", "log_std")

    def actor(dt):
        p = lambda k: sd[k].to(dt)
        x = torch.from_numpy(r["state"]).to(dt)
        for l in ("head.l", "l"):
            x = torch.relu(x @ p(l + ".weight").T + p(l + ".bias"))
        return torch.cat([x @ p(l + ".weight").T + p(l + ".bias") for l in last], -1)

    F.vs_exact(r["heads"], actor(torch.float64), actor(torch.float32), 1e-5, f"{ids(c)} heads")


@pytest.mark.parametrize("c, training", [(c, True) for c in CASES] + [(CASES[1], False), (CASES[3], False)], ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_stored_actions_are_the_streams_draws(c, training):
    """training=False: the plain tanh of the heads, and the counter still advances by T."""
    _, col, _, r, _ = rollout(c) if training else rollout(c, False)
    T, W, A = r["action"].shape
    assert col.stream == (SEED, T)
    assert np.abs(r["action"] - expected_actions(c[0], r["heads"].astype(np.float64), draws(W, T, A)[1], training)).max() <= 1e-5


def test_td3_uniform_phase():
    agent, _, col = make("td3", 17, 5, 64, 11, 3, initial_random_step=3)
    r, (u2, n) = run(col, 5), draws(17, 5, 3)
    assert agent.num_random_step == 3 and np.abs(r["action"][:3] - (2 * u2[:3] - 1)).max() <= 1e-5
    assert np.abs(r["action"][3:] - expected_actions("td3", r["heads"][3:].astype(np.float64), n[3:], True)).max() <= 1e-5
    col.run(5)
    assert agent.num_random_step == 3 and col.stream == (SEED, 10)


def test_a_rows_output_does_not_depend_on_the_tiling():
    a, b, again = rollout(CASES[3])[3], rollout(CASES[4])[3], rollout(CASES[3], again=1)[3]
    for k in a:
        assert np.array_equal(a[k], b[k][:, :17]), k
        assert np.array_equal(a[k], again[k]), k


@pytest.mark.parametrize("name", ["td3", "sac"])
def test_a_restored_collector_resumes_bit_for_bit(name):
    _, _, col = make(name, 17, 6, 64, 11, 3)
    run(col, 6)
    st = col.state()
    first = run(col, 6)
    _, _, fresh = make(name, 17, 6, 64, 11, 3)  # the same agent weights: make() seeds them
    fresh.set_state(st)
    again = run(fresh, 6)
    for k in first:
        assert np.array_equal(first[k], again[k]), k


@pytest.mark.parametrize("name", ["td3", "sac"])
def test_rows_feed_learn(name):
    W, T = 17, 8
    (dev, _, col), (twin, _, _) = make(name, W, T, 64, 11, 3), make(name, W, T, 64, 11, 3)
    rows = {k: v.reshape(W * T, -1) for k, v in run(col, T).items() if k != "heads"}
    noise = np.random.RandomState(3).randn(2 if name == "sac" else 1, 32, 3).astype(np.float32)
    results = []
    for agent, given in ((dev, None), (twin, rows)):
        np.random.seed(7)
        agent._noise_inject = noise
        results.append(agent.process(given, T))
        torch.cuda.synchronize()
    assert results[0] and results[0] == results[1]
    for net in ("actor", "critics"):
        for b in ("params", "m", "v"):
            assert torch.equal(getattr(dev._net, net)[b], getattr(twin._net, net)[b]), (net, b)


def test_refusals_name_what_is_eligible():
    from jorldy_amd import _lib as L
    from jorldy_amd import ops

    cap = ops.DEVROLL_AC_MAX_H
    for name, kw in (("ddpg", {}), ("sac", dict(actor="discrete_policy", critic="discrete_q_network")),
                     ("td3", dict(env_cls="DeviceCartPole", state_size=4, action_size=2)), ("td3", dict(hidden_size=24)), ("sac", dict(hidden_size=cap + 16)),
                     ("td3", dict(state_size=12))):
        with pytest.raises(ValueError, match="DeviceCollector runs the PPO agent on the MLP head only.*TD3 and the continuous SAC"):
            make(name, 4, 1, 64, 11, 3, **kw)
    agent, env, col = make("td3", 4, 1, 64, 11, 3)
    out = [torch.full((4, n), 7, dtype=dt, device="cuda") for n, dt in ((11, torch.float32), (3, torch.float32), (1, torch.float32), (11, torch.float32), (1, torch.uint8))]
    with pytest.raises(L.JhError, match="bad argument"):
        L.check(col.lib.jh_acnet_devroll_run(agent._net.h, env.h, 0, 1, 0, 0.1, SEED, 0, *[L.ptr(o) for o in out], None, L.stream_ptr()))
    torch.cuda.synchronize()
    assert all(bool((o == 7).all()) for o in out), "the output columns keep their sentinel"
