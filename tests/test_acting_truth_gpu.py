"""PPO's acting kernels against float64 at every dispatch edge of the collector (tests/acting_truth.py: CASES, dispatch): the persistent acting
kernel jh_act_persist_kernel<SP, NCH, D, PI> in each of its forms, and the two one-launch-per-step paths behind it, THROUGH the collector and its
acting-time capture -- the raw policy heads, V(s) and V(s') that PPO.learn takes over without recomputing them."""
import numpy as np
import pytest
import torch

import acting_truth as AT
import fp64_truth as F
from util import npy

pytestmark = pytest.mark.gpu

T = AT.T_STEPS
WORST = {}  # path -> {quantity: (e_ours, e_ref)} of the largest e_ours so far (printed per case)


@pytest.mark.parametrize("case", AT.CASES, ids=lambda c: c["name"])
def test_collector_acts_on_the_float64_policy(case, monkeypatch):
    """Two runs of T = 5 steps with a learn() in between (the second run acts with the weights learn() produced), capture on.  After each run:
      * NativeCollector.mode() is what dispatch(case) says (persistent / lookahead / split) and no run was handed over to per-step launches: the
        numbers below come from the path the case names;
      * the stored state / next_state / reward / done equal the env model's replay of the stored actions bit for bit (ScriptedVec.replay; the
        oracle's envs for the built-in ones);
      * captured h0, h1 (continuous), value, and next_value on the rows with done = 0 -- against V(state[w, t + 1]), V(next_state[w, T - 1]) for
        the last step -- are within max(1e-5, 2 x the error of torch-CPU float32) of the float64 module holding the agent's CURRENT weights,
        relative to the largest entry (fp64_truth.vs_exact); everything is finite, next_value on the done rows too;
      * continuous: stored actions in [-1, 1], the implied standard-normal draw (atanh(a) - mu) / std within +-6 on every row;
      * sharp discrete cases: the stored action is the float64 argmax on every row with p_max >= 1 - 1e-9, and those are >= 90 % of the rows.

    Measured on an MI355X, all 53 cases green in 4 s: the largest e_ours over the cases of a path (the torch-CPU-float32 e_ref of the same
    comparison), against the allowed max(1e-5, 2 e_ref):
      persistent kernel      h0 5.3e-7 (4.0e-7)   h1 5.2e-7 (5.4e-7)   value 1.4e-6 (5.4e-7)   next_value 1.3e-6 (1.1e-6)
      fused per-step launch  h0 4.2e-7 (3.8e-7)   h1 5.3e-7 (4.1e-7)   value 5.2e-7 (4.0e-7)   next_value 5.2e-7 (4.0e-7)
      separate-call forward  h0 2.3e-7 (2.2e-7)   h1 1.7e-7 (2.0e-7)   value 2.1e-7 (1.9e-7)   next_value 3.0e-7 (9.4e-7)
    What no case here can see: the persistent kernel zeroes the padding of W1 (q >= S) AND of the observation tile; either alone gives the same
    heads, so dropping one of the two guards changes no output (dropping both turns the SP 8 cases with S < 8 red).
    """
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.manager import NativeCollector

    for k in AT.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    want = AT.dispatch(case)
    W, S, A, H, cont = case["W"], case["S"], case["A"], case["H"], case["cont"]
    M = W * T
    torch.manual_seed(5)
    np.random.seed(5)
    agent = Agent("ppo", state_size=S, action_size=A, hidden_size=H, network=AT.network_name(case), n_step=T, batch_size=64, n_epoch=1, device="cuda",
                  backend="native", seed=3, lr_decay=False, num_workers=W)
    start64, _ = AT.sharp(case) if case["sharp"] else AT.policy(case)
    agent.network.load_state_dict({k: v.float() for k, v in start64.state_dict().items()})
    agent.memory.first_store = False
    env, model = AT.make_env(case), AT.make_model(case)
    col = NativeCollector(env, agent, W)
    assert col.capture
    worst = WORST.setdefault(want["path"], {})
    prev = None
    for run in range(AT.N_RUNS):
        sd = {k: v.detach().cpu().clone() for k, v in agent.network.state_dict().items()}
        if run == 0:
            assert all(torch.equal(sd[k], v.float()) for k, v in start64.state_dict().items())
        else:
            assert any(not torch.equal(sd[k], prev[k]) for k in sd), "learn() left the weights alone: the second run proves nothing"
        prev = sd
        m64, m32 = AT.modules_of(case, sd)
        col.run(T)
        torch.cuda.synchronize()
        mode = col.mode()
        assert (mode["persistent"], mode["lookahead"], mode["split"]) == (want["persist"], want["lookahead"], want["split"]), (mode, want)
        assert mode["handed_over"] == 0, mode
        store, st = agent.memory._store, agent._static
        assert store.size == M
        cols = {k: npy(store.column(k)[:M]).copy() for k in ("state", "action", "reward", "next_state", "done")}
        cap = {k: npy(st[k]).copy() for k in ("h0", "value", "next_value")}
        if cont:
            cap["h1"] = npy(st["h1"]).copy()
        # ---- the rollout is the env's
        action = cols["action"].reshape(W, T, A) if cont else cols["action"].reshape(W, T)
        state, next_state = cols["state"].reshape(W, T, S), cols["next_state"].reshape(W, T, S)
        r_state, r_next, r_rew, r_done = model.replay(action)
        done = cols["done"].reshape(W, T).astype(bool)
        assert state.dtype == np.float32 and np.array_equal(state, r_state), "state"
        assert np.array_equal(next_state, r_next), "next_state"
        assert np.array_equal(cols["reward"].reshape(W, T), r_rew), "reward"
        assert np.array_equal(done, r_done), "done"
        if case["kind"].startswith("scripted") and run == 0:
            assert done[:, 1].any() and done[:, T - 1].any()
        # ---- the captured numbers are the policy's
        assert all(np.isfinite(v).all() for v in cap.values())
        truth = AT.truths(case, m64, m32, state, next_state)
        go = torch.from_numpy(~done.reshape(-1))
        for q in ("h0", "h1", "value", "next_value"):
            if q not in truth:
                continue
            exact, ref32 = truth[q]
            ours = torch.from_numpy(cap[q]).reshape(exact.shape)
            if q == "next_value":
                ours, exact, ref32 = ours[go], exact[go], ref32[go]
            e_ours, e_ref = F.vs_exact(ours, exact, ref32, 1e-5, f"{case['name']} run {run} captured {q}")
            if e_ours >= worst.get(q, (-1.0, 0.0))[0]:
                worst[q] = (e_ours, e_ref)
        # ---- the stored actions are draws of it
        x64 = torch.from_numpy(state.reshape(M, S)).double()
        if cont:
            assert action.dtype == np.float32 and np.all(np.abs(action) <= 1.0)
            with torch.no_grad():
                mu, std, _ = m64(x64)
            a_cl = torch.clamp(torch.from_numpy(action.reshape(M, A)), -1 + 1e-7, 1 - 1e-7).double()  # (the reference's clamp, on float32: ppo.py:85-88)
            draw = (torch.atanh(a_cl) - mu) / std
            assert float(draw.abs().max()) <= 6.0, float(draw.abs().max())
        else:
            assert action.dtype == np.int64 and action.min() >= 0 and action.max() < A
            if case["sharp"]:
                with torch.no_grad():
                    pm, arg = AT.p_max(m64.raw(x64)[0])
                rows = pm >= AT.SHARP_P
                assert rows.mean() >= AT.SHARP_ROWS, rows.mean()
                assert np.array_equal(action.reshape(M)[rows], arg[rows])
        if run + 1 < AT.N_RUNS:
            res = agent.process(None, T * (run + 1))
            torch.cuda.synchronize()
            assert np.isfinite(res["actor_loss"]) and np.isfinite(res["critic_loss"]) and agent.memory.size == 0
    col.terminate()
    print(f"[acting truth] {case['name']} path {want['path']}: worst so far " + "  ".join(f"{q} {a:.2e} (fp32 {b:.2e})" for q, (a, b) in sorted(worst.items())))
