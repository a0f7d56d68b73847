"""Ape-X's device-resident actors (csrc/jh_devroll_q.hip through manager.DeviceCollector) against the host CartPole, the float64 network,
the exploration stream recomputed in numpy and the float64 window (apex_window_truth), at the smallest shapes at which the kernel can go
wrong: both kinds; H = 16 (one column tile), 48 (fewer tiles than waves for q, six for the 2H layer), 80 (tiles uneven over the waves), the
config's 512 and both caps; W = 1, 16, 17, 33; n_step 1, 3, 8 (T = 5 with n_step 8: the first run emits nothing); two runs per case, so
the window carries; T = 64, so episodes end inside windows; epsilon 0, 1, 0.4 with alpha 7 and 0, and training=False."""
import functools

import numpy as np
import pytest
import torch

import acting_truth as AT
import apex_window_truth as AW
import fp64_truth as F
import margins

pytestmark = pytest.mark.gpu

U = np.uint64
C1, FNV = U(0x9E3779B97F4A7C15), U(0x100000001B3)
SEED, ENV_SEED, GAMMA = 9, 5, 0.99
KEYS = ("state", "action", "reward", "next_state", "done", "priority")
#        network               H     W   n  T1  T2  eps  alpha training
CASES = [("dueling",            16,   1,  1,  3,  4, 0.4, 7.0, True), ("discrete_q_network", 16, 16, 3, 5, 6, 0.0, 7.0, True),
         ("dueling",            48,  17,  3,  7, 64, 0.4, 7.0, True), ("discrete_q_network", 48, 33, 8, 5, 12, 1.0, 0.0, True),
         ("dueling",            80,  33,  8,  5, 64, 0.4, 0.0, True), ("discrete_q_network", 80, 17, 1, 64, 2, 0.4, 7.0, False),
         ("dueling",            80,  17,  3,  6, 64, 0.4, 0.0, True), ("dueling",            80, 33, 3, 6, 64, 0.4, 0.0, True),
         ("dueling",           512,  16,  3,  4,  5, 0.4, 7.0, True), ("dueling",           816, 17, 3, 2, 4, 0.4, 7.0, True),
         ("discrete_q_network", 1216, 17, 3,  2,  4, 0.4, 7.0, True)]
ids = lambda c: "-".join(str(x) for x in c)


def make(network, H, W, n, eps, alpha, **kw):
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.network import Network
    from jorldy_amd.manager import DeviceCollector

    torch.manual_seed(11)
    m64 = Network(network, 4, 2, D_hidden=H, head="mlp").double()
    with torch.no_grad():
        for p in m64.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))  # every bias off zero
    sd = F.round_to_fp32_(m64).state_dict()
    agent = Agent("ape_x", state_size=4, action_size=2, hidden_size=H, network=network, head="mlp", n_step=n, batch_size=32, buffer_size=4096, gamma=GAMMA,
                  epsilon=eps, epsilon_alpha=alpha, epsilon_eval=0.3, start_train_step=0, device="cuda", **kw)
    agent._net.import_state({k: v.float() for k, v in sd.items()})
    agent._net.sync_target()
    env = ops.DeviceCartPole(W, ENV_SEED, "cuda")
    return agent, env, DeviceCollector(env, agent, seed=SEED), sd


def run(col, T, training=True):
    before = col.agent.memory.buffer_counter
    col.run(T, training=training)
    torch.cuda.synchronize()
    rows = col.agent.memory.buffer_counter - before
    return {k: col._out[k][:rows].cpu().numpy().copy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def rollout(c):
    """Two consecutive runs of the case -> (rows per run, every action taken [W, TT] (the last n_step from the saved window), float64 weights, agent)."""
    network, H, W, n, T1, T2, eps, alpha, training = c
    agent, env, col, sd = make(network, H, W, n, eps, alpha)
    runs = [run(col, T1, training), run(col, T2, training)]
    TT, blk = T1 + T2, col.state()["window"]
    assert col.window.position() == (TT, SEED, TT)
    slots = blk[24 + 4 * W * n * 4 + 8 * W * n:][: 4 * W * n].view(np.int32).reshape(W, n)  # header | states | q | reward | ACTION | done
    act = np.concatenate([r["action"].reshape(-1, W) for r in runs]).T
    tail = np.stack([slots[:, t % n] for t in range(TT - n, TT)], 1)
    return runs, np.concatenate([act, tail], 1), sd, agent


@pytest.mark.parametrize("c", CASES, ids=ids)
def test_rows_are_the_host_envs_the_streams_and_the_float64_windows(c):
    from jorldy_amd import ops

    network, H, W, n, T1, T2, eps, alpha, training = c
    runs, act, sd, agent = rollout(c)
    TT, E = T1 + T2, T1 + T2 - n
    # -- count and order: W * max(0, T - max(0, n_step - seen)) rows per run, time-major
    assert [len(r["priority"]) for r in runs] == [W * max(0, T1 - n), W * max(0, T2 - max(0, n - T1))] and agent.num_transitions == W * E
    rows = {k: np.concatenate([r[k].reshape((-1, W) + r[k].shape[1:]) for r in runs]).reshape(E, W, -1) for k in KEYS}
    # -- trajectory: the host env of the same seed on the actions taken
    env = ops.CartPoleVec(W, ENV_SEED)
    obs, rew, dn = np.empty((TT, W, 4), np.float32), np.empty((TT, W), np.float32), np.empty((TT, W), np.uint8)
    for t in range(TT):
        obs[t] = env.obs()
        _, rew[t], dn[t] = env.step(act[:, t])
    for e in range(E):
        assert np.array_equal(rows["reward"][e], rew[e:e + n].T) and np.array_equal(rows["done"][e], dn[e:e + n].T), e
        for ours, host, fresh in ((rows["state"][e], obs[e], dn[e - 1] == 1 if e else np.ones(W, bool)), (rows["next_state"][e], obs[e + n], dn[e + n - 1] == 1)):
            assert np.all(np.abs(ours - host) <= np.spacing(np.abs(host))) and np.array_equal(ours[fresh], host[fresh]), e
    if TT >= 64:
        assert (dn.sum(0) >= 2).any(), "several episodes end inside windows"
    # -- decision rule: the two uniforms per (t, env); explore -> the second's index, else greedy within the float32 forward's error
    s32 = np.concatenate([rows["state"][:n], rows["next_state"]])  # s_t as the kernel saw it, t = 0 .. TT - 1 (every case has E >= n)
    q64, q32 = AW.q_values(sd, network, s32), AW.q_values({k: v.float() for k, v in sd.items()}, network, s32).double()
    tol = max(1e-5, 2.0 * float((q32 - q64).abs().max() / q64.abs().max())) * float(q64.abs().max())
    margins.record(float((q32 - q64).abs().max()), tol, "torch-cpu-fp32 forward vs float64")
    q64 = q64.numpy()
    with np.errstate(over="ignore"):
        key = U(SEED) * FNV + np.arange(TT, dtype=U)[:, None] * C1 + np.arange(W, dtype=U)[None, :]
        u0, u1 = ((AT._mix(key * U(2) + U(k)) >> U(11)).astype(np.float64) / 9007199254740992.0 for k in (1, 2))
    eps_i = np.full(W, 0.3) if not training else np.float64(eps) ** (1 + (np.arange(W) / max(W - 1, 1)) * alpha) if W > 1 else np.full(1, eps)
    explore, taken = u0 < eps_i[None, :], np.take_along_axis(q64, act.T[..., None], -1)[..., 0]
    assert np.array_equal(act.T[explore], np.floor(u1 * 2).astype(np.int64)[explore])
    margins.leq((q64.max(-1) - taken)[~explore].max(initial=0.0), tol, "greedy actions: float64 q below the row's maximum")
    # -- priorities: the float64 window on the stored actions
    win, worst = AW.Windows(W, n, GAMMA), 0.0
    for t in range(TT):
        for w, row in enumerate(win.push(s32[t], act[:, t], rew[t].astype(np.float64), dn[t].astype(np.float64), taken[t])):
            if row is not None:
                assert row["action"] == rows["action"][t - n, w, 0] and np.array_equal(row["state"], rows["state"][t - n, w])
                worst = max(worst, abs(row["priority"] - rows["priority"][t - n, w, 0]))
    margins.leq(worst, sum(GAMMA ** i for i in range(n + 1)) * tol, "actor-side priorities vs the float64 window")


def test_a_rows_output_does_not_depend_on_the_tiling():
    a, b = rollout(CASES[6])[0], rollout(CASES[7])[0]
    for ra, rb in zip(a, b):
        for k in KEYS:
            assert np.array_equal(ra[k].reshape((-1, 17) + ra[k].shape[1:]), rb[k].reshape((-1, 33) + rb[k].shape[1:])[:, :17]), k


def test_buffer_state_is_what_store_device_leaves_and_feeds_learn():
    (dev, _, col, _), (twin, _, _, _) = make(*CASES[2][:4], 0.4, 7.0), make(*CASES[2][:4], 0.4, 7.0)
    for T in (7, 64):
        r = run(col, T)
        cols = {k: torch.from_numpy(r[k]).cuda() for k in KEYS[:5]}
        twin.memory.store_device(cols, {k: v[:1].cpu().numpy() for k, v in cols.items()}, priorities=torch.from_numpy(r["priority"]).cuda())
    a, b = dev.memory, twin.memory
    assert (a.buffer_index, a.buffer_counter, a.max_priority) == (b.buffer_index, b.buffer_counter, b.max_priority) and a.buffer_counter == 17 * 68
    assert np.array_equal(a._tree.dump(), b._tree.dump())
    np.random.seed(7)
    res = dev.process(None, 4)  # no staging ring was ever made; one learn() at learn_period 4
    np.random.seed(7)
    ref = twin.process(None, 4)
    torch.cuda.synchronize()
    assert res["loss"] == ref["loss"] and res["num_transitions"] == 17 * 68 and torch.equal(dev._net.params, twin._net.params)


def test_a_restored_collector_resumes_bit_for_bit():
    _, _, col, _ = make("dueling", 48, 17, 3, 0.4, 7.0)
    run(col, 5)
    st = col.state()
    first = run(col, 9)
    col.set_state(st)
    again = run(col, 9)
    for k in KEYS:
        assert np.array_equal(first[k], again[k]), k


def test_refusals():
    from jorldy_amd import ops
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import DeviceCollector

    cp = ops.DeviceCartPole(4, 0, "cuda")
    for name, kw in (("r2d2", {}), ("ape_x", dict(state_size=[4, 84, 84], head="cnn", network="dueling")), ("ape_x", dict(hidden_size=832, network="dueling"))):
        with pytest.raises(ValueError, match="DeviceCollector runs the PPO agent on the MLP head only"):
            DeviceCollector(cp, Agent(name, **{**dict(state_size=4, action_size=2, hidden_size=64, device="cuda"), **kw}))
