"""The discrete SAC's and DQN's device-resident actors (csrc/jh_devroll_disc.hip through manager.DeviceCollector) against the host CartPole, the
float64 network and the exploration stream recomputed in numpy, at the smallest shapes at which the kernel can go wrong: W = 1, 15, 17, 33 (a
row, a tile less / plus one row, three tiles); H = 16 (one k chunk: three waves idle in the tail), 80 (five chunks over four waves) and the
cap (all of the LDS); T = 1, 2 and 160 (every env resets inside the launch).  DeviceCartPole has two actions: the tail's four column tiles and
the wider lane groups (A = 3, 16, 17, 64) are driven through the C entry's probe flag, which leaves the env where it is."""
import numpy as np
import pytest
import torch

import acting_truth as AT
import fp64_truth as F
from jorldy_amd import _lib as L
from jorldy_amd import ops
from jorldy_amd.core.agent import Agent
from jorldy_amd.core.network import Network
from jorldy_amd.manager import DeviceCollector
from util import npy

pytestmark = pytest.mark.gpu
U, C1, FNV = np.uint64, np.uint64(0x9E3779B97F4A7C15), np.uint64(0x100000001B3)
SEED, ENV_SEED, EPS, EPS_EVAL, LONG = 9, 5, 0.5, 0.05, 160
CASES = [("sac", 1, 1, 16), ("dqn", 15, 2, 16), ("sac", 17, LONG, 80), ("sac", 33, LONG, 80), ("dqn", 17, LONG, 80), ("dqn", 33, LONG, 80), ("dqn", 17, 2, "cap")]  # agent, W, T, H
ids = lambda v: "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def weights(network, A, H):  # -> float64 state_dict of the reference module, fp32-representable, every bias off zero
    torch.manual_seed(11)
    m = Network(network, 4, A, D_hidden=H, head="mlp").double()
    for p in (p for p in m.parameters() if p.dim() == 1):
        p.data.add_(0.05 * torch.randn_like(p))
    return F.round_to_fp32_(m).state_dict()


def make(name, W, H, env_cls="DeviceCartPole", **kw):  # -> (agent, env, collector, float64 weights); with `kw` (the refusals) the agent keeps its own weights
    H = ops.DEVROLL_DISC_MAX_H if H == "cap" else H
    own = dict(actor="discrete_policy", critic="discrete_q_network") if name == "sac" else dict(epsilon_init=EPS, epsilon_eval=EPS_EVAL, run_step=1000)
    agent = Agent(name, **{**dict(state_size=4, action_size=2, hidden_size=H, batch_size=32, buffer_size=8192, start_train_step=4, lr_decay=False, device="cuda"), **own, **kw})
    sd = None if kw else weights("discrete_policy" if name == "sac" else "discrete_q_network", 2, H)
    if sd is not None:
        agent._net.import_state({k: v.float() for k, v in sd.items()})
    env = ops.DeviceCartPole(W, ENV_SEED, "cuda") if env_cls == "DeviceCartPole" else ops.DeviceControl(W, 4, 2, ENV_SEED, "cuda")
    return agent, env, DeviceCollector(env, agent, seed=SEED), sd


def run(col, T, training=True):
    col.capture_heads = True
    col.run(T, training=training)
    return {k: npy(v[: col.env.W * T]).copy().reshape(T, col.env.W, -1) for k, v in col._out.items()}


def logits_are_the_float64_networks(sd, x, heads, what):
    layer = lambda x, l, dt: x @ sd[l + ".weight"].to(dt).T + sd[l + ".bias"].to(dt)
    net = lambda dt: layer(torch.relu(layer(torch.relu(layer(torch.as_tensor(x).to(dt), "head.l", dt)), "l", dt)), "pi" if "pi.weight" in sd else "q", dt)
    F.vs_exact(heads, net(torch.float64), net(torch.float32), 1e-5, what + " logits")


def actions_are_the_streams_draws(action, heads, pi, training, eps, ctr=0):
    """action [T, W], heads [T, W, A] as captured.  No row of these seeds has its u within 1e-6 of a boundary of the float64 CDF: none is left out."""
    (T, W, A), z = heads.shape, heads.astype(np.float64)
    with np.errstate(over="ignore"):
        key = U(SEED) * FNV + (U(ctr) + np.arange(T, dtype=U)[:, None]) * C1 + np.arange(W, dtype=U)[None, :]
        u, u1, u2 = ((AT._mix(k) >> U(11)).astype(np.float64) / 9007199254740992.0 for k in (key, key * U(2) + U(1), key * U(2) + U(2)))
    greedy = heads.argmax(-1)  # the first index of the largest float32 value
    if not pi:
        assert np.array_equal(action, np.where(u1 < eps, np.floor(u2 * A).astype(np.int64), greedy))
    elif not training:
        assert np.array_equal(action, greedy)
    else:
        p = np.exp(z - z.max(-1, keepdims=True))
        cdf = np.cumsum(p / p.sum(-1, keepdims=True), -1)[..., :-1]
        assert (np.abs(u[..., None] - cdf).min(-1) > 1e-6).all() and np.array_equal(action, (u[..., None] >= cdf).sum(-1))


@pytest.mark.parametrize("c, training", [(c, True) for c in CASES] + [(CASES[2], False), (CASES[4], False)], ids=ids)
def test_rows_are_the_float64_networks_the_streams_and_the_host_envs(c, training):
    """DQN: one epsilon for all rows (epsilon, or epsilon_eval when not training), decided per env row.  The counter advances by T either way."""
    _, _, col, sd = make(c[0], c[1], c[3])
    r, (_, W, T, _) = run(col, c[2], training), c
    assert col.stream == (SEED, T)
    logits_are_the_float64_networks(sd, r["state"], r["heads"], ids(c))
    actions_are_the_streams_draws(r["action"][..., 0], r["heads"], c[0] == "sac", training, EPS if training else EPS_EVAL)
    env, done = ops.CartPoleVec(W, ENV_SEED), r["done"][..., 0].astype(bool)
    for t in range(T):
        obs = env.obs()
        nxt, rew, dn = env.step(r["action"][t, :, 0])
        assert np.array_equal(dn.astype(bool), done[t]) and np.array_equal(rew, r["reward"][t, :, 0]), t
        for ours, host in ((r["state"][t], obs), (r["next_state"][t], nxt)):
            assert np.all(np.abs(ours - host) <= np.spacing(np.abs(host))), t
        if t + 1 < T:
            assert np.array_equal(r["state"][t + 1][~done[t]], r["next_state"][t][~done[t]])
            assert np.array_equal(r["state"][t + 1][done[t]], env.obs()[done[t]]), "the reset observation is the host's, bit for bit"
    assert T < LONG or done.any(0).all(), "every env resets inside the launch"


@pytest.mark.parametrize("name", ["sac", "dqn"])
def test_a_rows_output_depends_on_neither_the_tiling_nor_a_restore(name):
    col, wide, fresh = (make(name, W, 80)[2] for W in (17, 33, 17))  # three envs and collectors, the same weights
    run(col, 5), run(wide, 5)
    fresh.set_state(col.state())
    first, other, again = run(col, 40), run(wide, 40), run(fresh, 40)
    for k in first:
        assert np.array_equal(first[k], again[k]) and np.array_equal(first[k], other[k][:, :17]), k
    assert first["done"].any(), "episodes end and restart inside the compared runs"


@pytest.mark.parametrize("name", ["sac", "dqn", "double"])
def test_rows_feed_learn(name):
    """Epsilon decays as process() defines it: by (step - time_t) * epsilon_delta per call once a learn() has run: T per call here, not W * T."""
    (agent, _, col, _), W, T = make(name, 17, 80), 17, 8
    np.random.seed(7)
    for i in (1, 2, 3):  # eager, captured, replayed
        col.run(T)
        res = agent.process(None, i * T)
        assert res and all(np.isfinite(v) for v in res.values()) and agent.memory.size == i * W * T
    if name != "sac":
        assert agent.num_learn == 3 and agent.epsilon == pytest.approx(EPS - 3 * T * (EPS - 0.1) / 100, abs=1e-12)


@pytest.mark.parametrize("A", [3, 16, 17, 64])
def test_tail_and_draws_beyond_the_envs_two_actions(A):
    """The probe flag of jh_devroll_disc_run: logits and actions only, the env read but not stepped, every timestep from the same states."""
    W, T, H = 17, 3, 80
    sd = weights("discrete_policy", A, H)
    net = ops.RainbowNet(4, A, 1, H, "mlp", 1, "cuda", kind="pi")
    net.import_state({k: v.float() for k, v in sd.items()})
    env, s = ops.DeviceCartPole(W, ENV_SEED, "cuda"), np.random.RandomState(A).randn(W, 4)
    env.set_state(s=s)
    heads, action = torch.empty(T * W, A, device="cuda"), torch.empty(T * W, dtype=torch.int64, device="cuda")
    for mode, training in ((0, 1), (0, 0), (1, 1)):
        L.check(net.lib.jh_devroll_disc_run(net.h, L.ptr(net.params), env.h, T, mode, training, EPS, SEED, 4, None, L.ptr(action), None, None, None, L.ptr(heads), 1, L.stream_ptr()))
        h = npy(heads).reshape(T, W, A)
        logits_are_the_float64_networks(sd, np.broadcast_to(s.astype(np.float32), (T, W, 4)).copy(), h, f"A {A}")
        actions_are_the_streams_draws(npy(action).reshape(T, W), h, mode == 0, training, EPS, ctr=4)
    assert np.array_equal(env.state()["s"], s), "the probe leaves the env where it is"


def test_refusals_and_bad_arguments():
    for name, kw in (("dueling", dict(network="dueling")), ("multistep", dict(n_step=3)), ("dqn", dict(state_size=[4, 84, 84], head="cnn")), ("sac", dict(hidden_size=24)),
                     ("dqn", dict(hidden_size=ops.DEVROLL_DISC_MAX_H + 16)), ("sac", dict(env_cls="DeviceControl")), ("dqn", dict(env_cls="DeviceControl"))):
        with pytest.raises(ValueError, match="DeviceCollector runs the PPO agent on the MLP head only.*TD3 and the continuous SAC.*SACDiscrete / DQN / Double"):
            make(name, 4, 64, **kw)
    agent, env, col, _ = make("sac", 4, 64)
    out = [torch.full((4, n), 7, dtype=dt, device="cuda") for n, dt in ((4, torch.float32), (1, torch.int64), (1, torch.float32), (4, torch.float32), (1, torch.uint8), (2, torch.float32))]
    with pytest.raises(L.JhError, match="bad argument"):
        L.check(col.lib.jh_devroll_disc_run(agent._net.h, L.ptr(agent._net.params), env.h, 0, 0, 1, 0.0, SEED, 0, *[L.ptr(o) for o in out], 0, L.stream_ptr()))
    assert all(bool((o == 7).all()) for o in out), "the output columns keep their sentinel"
