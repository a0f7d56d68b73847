"""RND-PPO without a GPU: the C ABI's new entries, the padded parameter count, the registries, the loud failure without a device, the
eligibility sentence, the mirror networks against the fixtures' recorded state_dicts and initial weights, the float64 truth of
tests/rnd_truth.py against both learns of the three small fixtures of tools/gen_golden_rnd.py, the proof that no sweep case of the GPU test
sits on a discontinuity, and the curve fixture under the GPU curve test's criterion."""
import json
import os
import re
import warnings

import numpy as np
import pytest
import torch

import rnd_truth as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("jh_rndnet_param_count_for", "jh_rndnet_create", "jh_rndnet_destroy", "jh_rndnet_segment_count", "jh_rndnet_segment", "jh_rndnet_trainable_floats",
           "jh_rndnet_set_hyper", "jh_rndnet_set_lr", "jh_rndnet_stats_floats", "jh_rndnet_stats_get", "jh_rndnet_stats_set", "jh_rndnet_obs_update", "jh_rndnet_reward",
           "jh_rndnet_update", "jh_rnd_adv_mix", "jh_rnd_ppo_loss_packed")
FIX_TOL = dict(rtol=1e-5, atol=1e-5)  # the project's fixture tolerance


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_carry_the_new_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/jorldy_hip.h"
        assert hasattr(lib, name) and name in _lib.exported_names()
    for ref in ("rnd_ppo.py:", "rnd.py:"):
        assert ref in src, "the header cites the reference's lines"
    tg = open(os.path.join(ROOT, "jorldy_amd", "csrc", "jh_tgemm.h")).read()
    assert "rnd" not in tg.lower(), "no new call-site tag: the module's contractions run under jh_tgemm_dense"
    csrc = os.path.join(ROOT, "jorldy_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "jh_rnd.hip" in mk and "jh_curiosity.h" in mk
    # one copy of what the two modules share: both translation units include the header, neither defines the shared kernels itself
    shared = ("cur_col_sum", "cur_rms_merge", "jh_cur_obs_update_kernel", "jh_cur_prep_kernel", "jh_cur_bn_act_kernel", "jh_cur_bn_act_bwd_kernel", "jh_cur_reward_kernel")
    head = open(os.path.join(csrc, "jh_curiosity.h")).read()
    for unit in ("jh_icm.hip", "jh_rnd.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "jh_curiosity.h"' in text
        for name in shared:
            assert re.search(r"\b" + name + r"\b", head)
            assert not re.search(r"(__global__|__device__)[^;{]*\b" + name + r"\s*\(", text), f"{unit} defines {name} itself"
    assert '#include "jh_policy_head.h"' in open(os.path.join(csrc, "jh_rnd.hip")).read()


def test_param_count_is_the_padded_sum_of_the_modules_tensors(lib):
    """jh_rndnet_param_count_for is host-only: two trunks of fc1 [H][S], [H], fc2 [256][H], [256] and, with batch norm, two vectors for each of the
    four batch norms; every segment starts 16-byte aligned."""
    up4 = lambda x: (x + 3) // 4 * 4
    for S, H in ((3, 8), (4, 32), (11, 20)):
        trunk = up4(H * S) + up4(H) + up4(256 * H) + up4(256)
        bn = 2 * up4(H) + 2 * up4(256)
        assert lib.jh_rndnet_param_count_for(S, H, 0) == 2 * trunk
        assert lib.jh_rndnet_param_count_for(S, H, 1) == 2 * (trunk + bn)
        cfg = D.config(S, H)
        assert lib.jh_rndnet_param_count_for(S, H, 1) == sum(up4(int(np.prod(sh))) for sh in D.shapes(cfg).values())
    for bad in ((0, 8, 1), (3, 6, 1), (3, 0, 1)):
        assert lib.jh_rndnet_param_count_for(*bad) == -1, bad


def test_registries():
    from jorldy_amd.core.agent import PPO, Agent, agent_dict
    from jorldy_amd.core.agent.rnd_ppo import RND_PPO
    from jorldy_amd.core.network import RND_MLP, ContinuousPolicySeparateValue, DiscretePolicySeparateValue, network_dict

    assert agent_dict["rnd_ppo"] is RND_PPO and issubclass(RND_PPO, PPO) and network_dict["rnd_mlp"] is RND_MLP
    assert network_dict["discrete_policy_separate_value"] is DiscretePolicySeparateValue and network_dict["continuous_policy_separate_value"] is ContinuousPolicySeparateValue
    with pytest.raises(RuntimeError, match="parameter container"):
        RND_MLP(4, 2, 8, 0.99, D_hidden=16)(torch.zeros(2, 4))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("rnd_ppo", state_size=4, action_size=2, network="discrete_policy_separate_value")


INELIGIBLE = [("rnd_cnn", dict(rnd_network="rnd_cnn")), ("rnd_multi", dict(rnd_network="rnd_multi")), ("cnn head", dict(head="cnn", state_size=(4, 84, 84))),
              ("multi head", dict(head="multi", state_size=[(4, 84, 84), 5])), ("one value head", dict(network="discrete_policy_value")),
              ("continuous, one value head", dict(network="continuous_policy_value")), ("the default network", dict(network=None)), ("hidden 30", dict(hidden_size=30)),
              ("rmsprop", dict(optim_config={"name": "rmsprop"})), ("weight decay", dict(optim_config={"name": "adam", "weight_decay": 1e-4})),
              ("grad_sync", dict(grad_sync=object())), ("oversize batch", dict(batch_size=8193))]


@pytest.mark.parametrize("label,over", INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_configurations_raise_the_eligibility_sentence_before_any_gpu_use(label, over):
    """The check comes BEFORE the device check: the sentence is raised on a machine without a GPU too, and names the library."""
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.rnd_ppo import RND_ELIGIBLE

    kw = dict(state_size=4, action_size=2, network="discrete_policy_separate_value")
    kw.update(over)
    if kw["network"] is None:
        del kw["network"]
    with pytest.raises(ValueError) as e:
        Agent("rnd_ppo", **kw)
    assert str(e.value).startswith(RND_ELIGIBLE) and "libjorldy_hip" in RND_ELIGIBLE


@pytest.mark.parametrize("name", D.FIXTURES)
def test_mirror_networks_have_the_fixtures_keys_shapes_and_order(name):
    """Keys, order and shapes of both containers' state_dicts equal the recorded lists (the module: 35 keys with batch norm, 15 without; 23 / 15
    parameters, of which only the predictor's get a gradient); the small fixtures also hold the initial weights of the reference's agent under
    one torch.manual_seed: the containers, built in the reference's order, draw the same."""
    from jorldy_amd.core.network import Network

    fx = D.load_fixture(name)
    sp = fx.spec
    kw = D.agent_kwargs(sp)
    torch.manual_seed(fx.init_seed)
    net = Network(kw["network"], fx.S, fx.A, D_hidden=fx.H, head="mlp")
    rnd = Network("rnd_mlp", fx.S, fx.A, fx.W, D.GAMMA_I, sp["on"], sp["on"], sp["on"], D_hidden=fx.H)
    heads = ["mu", "log_std"] if fx.cont else ["pi"]
    assert list(net.state_dict()) == list(fx.sd0) == [f"{m}.{t}" for m in ["head.l", "l"] + heads + ["v", "v_i"] for t in ("weight", "bias")]
    assert list(rnd.state_dict()) == list(fx.rnd0) and len(fx.rnd0) == (35 if sp["on"] else 15)
    for sd, prefix in ((net.state_dict(), "shape/"), (rnd.state_dict(), "shape/rnd.")):
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(int(s) for s in fx.z[prefix + k]), k
    params = dict(rnd.named_parameters())
    assert len(params) == (23 if sp["on"] else 15) and [k for k, p in params.items() if p.requires_grad] == sorted(D.trainable(fx.cfg), key=list(params).index)
    assert list(D.shapes(fx.cfg)) == [k for k in params if k.split(".")[0] not in ("rms_obs", "rms_ri", "rff")]
    if not fx.recipe:
        for sd, prefix in ((net.state_dict(), "init/"), (rnd.state_dict(), "init_rnd/")):
            for k, v in sd.items():
                # (orthogonal_ factorises with LAPACK, whose roundings follow the thread count: the same draws, equal to the fixture tolerance)
                np.testing.assert_allclose(v.numpy(), fx.z[prefix + k], **FIX_TOL, err_msg=f"{name} initial {k}")
        assert abs(float(net.state_dict()["v_i.weight"].norm()) - 0.01) < 1e-6 and abs(float(net.state_dict()["v.weight"].norm()) - 0.01) < 1e-6, "gain 0.01 on both value heads"


@pytest.mark.parametrize("name", D.SMALL)
def test_truth_reproduces_both_learns_of_the_small_fixtures(name):
    """tests/rnd_truth.py in float64, started from the fixture's starting state_dicts and continued over both learns with its own two Adams,
    against every record (rtol and atol 1e-5): the pre-pass tensors r_i, value, v_i, the mixed advantage, ret, ret_i, log pi_old; every
    minibatch's actor, both critic losses, entropy and the module's loss; the clipped gradients of both networks at the first and the last
    minibatch; the statistics block after each learn."""
    warnings.filterwarnings("ignore", category=UserWarning)
    fx = D.load_fixture(name)
    z, state = fx.z, D.truth_state(fx)
    assert fx.learns == 2 and 2 <= fx.M % fx.B < fx.B, "two learns, a ragged last minibatch of at least two rows"
    for k in range(fx.learns):
        out = D.learn_truth(fx, k, state)
        for key, v in out["pre"].items():
            np.testing.assert_allclose(v.numpy().reshape(-1), z[f"l{k}/pre/{key}"].reshape(-1), **FIX_TOL, err_msg=f"{name} l{k} pre-pass {key}")
        seen = 0
        for i, mb in enumerate(out["mb"]):
            for key in ("actor_loss", "critic_e_loss", "critic_i_loss", "entropy_loss", "rnd_loss"):
                np.testing.assert_allclose(mb[key], float(z[f"l{k}/mb{i}/{key}"]), **FIX_TOL, err_msg=f"{name} l{k} mb{i} {key}")
            if f"l{k}/mb{i}/grad/l.weight" in z.files:
                seen += 1
                for tag, grads in (("grad", mb["grad"]), ("rnd_grad", mb["rnd_grad"])):
                    rec = fx.sub(f"l{k}/mb{i}/{tag}/")
                    assert list(rec) == list(grads)
                    for kk, g in grads.items():
                        np.testing.assert_allclose(fx.thin(g.numpy()).reshape(-1), rec[kk].reshape(-1), **FIX_TOL, err_msg=f"{name} l{k} mb{i} {tag} {kk}")
        assert seen == 2
        end = fx.sub(f"l{k}/rnd1/")
        for key in D.BLOCK_KEYS:
            if key in end:
                np.testing.assert_allclose(fx.thin(state["blk"][key]).reshape(-1), end[key].reshape(-1), rtol=1e-5, atol=2.1 * fx.lr if "running_mean" in key else 1e-5,
                                           err_msg=f"{name} l{k} block {key}")  # the running means carry the fc biases in front of them, which travel by Adam's steps on rounding noise
        if fx.spec["on"]:
            assert int(end["bn2_target_mlp.num_batches_tracked"]) == (k + 1) * (1 + fx.n_minibatch())


def test_fixture_switches_take_every_branch():
    """Across the four fixtures: both policy types, episodic and non-episodic, standardisation on and off, the switches on and off, non_extrinsic;
    the continuous one has saturated actions and a clamped mu."""
    sp = D.SPECS
    assert {s["cont"] for s in sp.values()} == {s["non_episodic"] for s in sp.values()} == {s["std"] for s in sp.values()} == {s["on"] for s in sp.values()} == {True, False}
    assert sp["rnd_plain"]["non_extrinsic"] and not sp["rnd_plain"]["on"]
    assert dict(D.CURVE_CONFIG["agent"], optim_config=None) == dict({k: v for k, v in D.agent_kwargs(sp["rnd_cartpole"]).items() if k not in ("run_step", "num_workers", "non_extrinsic")},
                                                                   optim_config=None, lr_decay=True), "rnd_cartpole is config.rnd_ppo.cartpole"
    fx = D.load_fixture("rnd_continuous")
    c = fx.cols(0)
    assert (np.abs(c["action"]) == 1.0).any(), "saturated actions"
    P = {k: torch.from_numpy(np.asarray(v)).double() for k, v in fx.sd0.items()}
    assert float(D.policy_heads(P, torch.from_numpy(c["state"]).double(), True)[:, 0].abs().max()) > 5.0, "a mu past the clamp"


def test_no_sweep_case_sits_on_a_discontinuity():
    """The float64 truth alone, over EVERY case of the GPU sweeps (none is dropped): the smallest distance from a ratio at the clip edge, a value
    move at +-eps, two equal critic means, a pre-activation at 0 and a normalised observation at +-5 stays above rnd_truth.CLEAR; the variants do
    what they are named for."""
    warnings.filterwarnings("ignore", category=UserWarning)
    n = 0
    for tag, cfg, b in D.cases():
        w, blk, s2, idx = D.update_case(tag, cfg, b)
        m = D.module_margins(D.update(cfg, w, blk, s2[idx], 0.02))
        assert all(m[k] >= D.CLEAR[k] for k in m), (tag, m)
        n += 1
    assert {b for _, _, b in D.cases()} == set(D.UPDATE_ROWS + (17, 64)) and {c["S"] for _, c, _ in D.cases()} == set(D.UPDATE_S) and {c["H"] for _, c, _ in D.cases()} == set(D.UPDATE_H)
    for tag, cfg, M in D.reward_cases():
        w, blk, s2 = D.case_inputs(tag, cfg, M)
        m = D.module_margins(D.reward_pass(cfg, w, blk, s2))
        assert all(m[k] >= D.CLEAR[k] for k in m), (tag, m)
        n += 1
    for c in D.loss_cases():
        x = D.loss_case(*c)
        r = D.ppo_loss(c[1], x["heads"], c[2], x["action"], x["adv"], x["ret"], x["ret_i"], x["v_old"], x["vi_old"], x["lp_old"], x["eps"], x["vf"], x["ent"])
        m = D.loss_margins(r, x["eps"])
        assert all(m[k] >= D.CLEAR[k] for k in m), (c[0], m)
        if c[4] == "clipped":
            assert bool(((r["rows"]["ratio"] < 1 - x["eps"]) | (r["rows"]["ratio"] > 1 + x["eps"])).all()), c[0]
        if c[4] == "critic":
            assert r["means"]["c2"] > r["means"]["c1"] and r["means"]["i2"] > r["means"]["i1"], c[0]
        if c[4] == "plain" and c[3] >= 63:
            assert bool((r["rows"]["ratio"] < 1 - x["eps"]).any()) and bool((r["rows"]["ratio"] > 1 + x["eps"]).any()) and bool((r["rows"]["dv"].abs() < x["eps"]).any())
        n += 1
    assert n == len(D.cases()) + len(D.reward_cases()) + len(D.loss_cases()) == 34 + 11 + 126, "every case of the sweeps, none dropped"


def test_curve_fixture_meets_the_gpu_tests_criterion():
    """The reference's own three seeds under the criterion the GPU curve test applies to ours: every seed gains at least 3x from the first
    iteration to the mean of the last five, and the seeds' mean end lies within the seed spread of the reference's end (its own: the margin is
    not degenerate, and no single seed is further from the mean than the spread)."""
    with open(os.path.join(D.GOLDEN, "curves_reference_rnd_ppo.json")) as f:
        fx = json.load(f)
    assert fx["config"] == json.loads(json.dumps(D.CURVE_CONFIG)), "the fixture was generated for another configuration: rerun tools/gen_golden_rnd.py --only curves"
    ref = fx["rnd_ppo_cartpole"]["reference"]
    assert len(ref) == 3 and all(len(c) == D.CURVE_CONFIG["iterations"] for c in ref)
    r_end, spread = D.curve_criterion(ref)
    assert min(D.curve_end(c) / c[0] for c in ref) >= 3.0
    assert 0.0 < spread < r_end and abs(float(np.mean([D.curve_end(c) for c in ref])) - r_end) <= spread and all(abs(D.curve_end(c) - r_end) <= spread for c in ref)
