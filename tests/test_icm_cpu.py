"""ICM-PPO without a GPU: the C ABI's new entries, the padded parameter count, the registries, the loud failure without a device, the eligibility
sentence, the parameter container against the fixture's recorded state_dict, the float64 truth of tests/icm_truth.py against every record of
every fixture of tools/gen_golden_icm.py, the filter's aliasing, and the float32 comparator's errors that the GPU test's bounds are made of."""
import os
import re

import numpy as np
import pytest
import torch

import icm_truth as D
import margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("param_count_for", "create", "destroy", "segment_count", "segment", "set_hyper", "set_lr", "stats_floats", "stats_get", "stats_set", "obs_update", "reward",
           "update")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_header_library_and_binding_carry_the_new_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    for e in ENTRIES:
        name = "jh_icmnet_" + e
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} is not declared in include/jorldy_hip.h"
        assert hasattr(lib, name) and name in _lib.exported_names()
    for ref in ("icm_ppo.py:", "icm.py:", "utils.py:", "rnd.py:"):
        assert ref in src, "the header cites the reference's lines"
    assert lib.jh_abi_version() == 2
    tg = open(os.path.join(ROOT, "jorldy_amd", "csrc", "jh_tgemm.h")).read()
    assert "icm" not in tg.lower(), "no new call-site tag: the ICM's contractions run under jh_tgemm_dense"
    assert "jh_icm.hip" in open(os.path.join(ROOT, "jorldy_amd", "csrc", "Makefile")).read()


def test_param_count_is_the_padded_sum_of_the_modules_tensors(lib):
    """jh_icmnet_param_count_for is host-only.  The tensors written out from icm.py:8-18, 99-118, 181-188 at the smallest shapes, for both policy
    types, with and without batch norm; every segment starts 16-byte aligned."""
    up4 = lambda x: (x + 3) // 4 * 4
    total = lambda shapes: sum(up4(r * c) for r, c in shapes)
    lin = lambda out, inp: [(out, inp), (1, out)]
    S, H, F = 3, 8, 256
    for cont, A in ((0, 2), (0, 3), (1, 1), (1, 3)):
        a = A if cont else 1
        net = lin(H, S) + lin(F, H) + lin(H, F + a) + lin(F, H + a) + lin(H, 2 * F) + lin(A, H)
        bn = [(1, H), (1, H), (1, F), (1, F), (1, H), (1, H)]
        assert lib.jh_icmnet_param_count_for(S, H, A, cont, 0) == total(net), (cont, A)
        assert lib.jh_icmnet_param_count_for(S, H, A, cont, 1) == total(net + bn), (cont, A)
    for bad in ((0, 8, 2, 0, 1), (3, 6, 2, 0, 1), (3, 8, 40, 0, 1), (3, 8, 20, 1, 1), (3, 8, 0, 0, 1), (3, 8, 2, 2, 1)):
        assert lib.jh_icmnet_param_count_for(*bad) == -1, bad


def test_registries():
    from jorldy_amd.core.agent import ICM_PPO, PPO, Agent, agent_dict
    from jorldy_amd.core.network import ICM_MLP, network_dict

    assert agent_dict["icm_ppo"] is ICM_PPO and issubclass(ICM_PPO, PPO) and network_dict["icm_mlp"] is ICM_MLP
    with pytest.raises(RuntimeError, match="parameter container"):
        ICM_MLP(4, 2, 8, 0.99, 0.1, "discrete", D_hidden=16)(torch.zeros(2, 4), torch.zeros(2, 1), torch.zeros(2, 4))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            Agent("icm_ppo", state_size=4, action_size=2)


INELIGIBLE = [("icm_cnn", dict(icm_network="icm_cnn")), ("icm_multi", dict(icm_network="icm_multi")), ("lamb", dict(lamb=0.5)), ("cnn head", dict(head="cnn", state_size=(4, 84, 84))),
              ("hidden 100", dict(hidden_size=100)), ("rmsprop", dict(optim_config={"name": "rmsprop"})), ("weight decay", dict(optim_config={"name": "adam", "weight_decay": 1e-4})),
              ("separate value", dict(network="continuous_policy_separate_value")), ("discrete separate value", dict(network="discrete_policy_separate_value")),
              ("oversize batch", dict(batch_size=8193))]


@pytest.mark.parametrize("label,over", INELIGIBLE, ids=[c[0] for c in INELIGIBLE])
def test_ineligible_configurations_raise_the_eligibility_sentence_before_any_gpu_use(label, over):
    """The check comes BEFORE the device check: the sentence is raised on a machine without a GPU too, and names the library."""
    from jorldy_amd.core.agent import Agent
    from jorldy_amd.core.agent.icm_ppo import ICM_ELIGIBLE

    kw = dict(state_size=4, action_size=2)
    kw.update(over)
    with pytest.raises(ValueError) as e:
        Agent("icm_ppo", **kw)
    assert str(e.value).startswith(ICM_ELIGIBLE) and "libjorldy_hip" in ICM_ELIGIBLE


@pytest.mark.parametrize("name", D.FIXTURES)
def test_container_state_dict_is_the_references(name):
    """Keys, order and shapes of the container's state_dict equal the recorded list (34 keys with batch norm, 19 without); 25 / 19 parameters,
    the first seven without gradient; the same torch.manual_seed gives torch's default initialisation in the reference's order."""
    from jorldy_amd.core.network import Network

    fx = D.load_fixture(name)
    mk = lambda: Network("icm_mlp", fx.S, fx.A, fx.W, 0.99, 0.1, "continuous" if fx.cont else "discrete", fx.on, fx.on, fx.on, D_hidden=fx.H)
    torch.manual_seed(3)
    m = mk()
    sd = m.state_dict()
    rec = [k[len("shape/icm."):] for k in fx.z.files if k.startswith("shape/icm.")]
    assert list(sd) == rec and len(sd) == (34 if fx.on else 19)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(s) for s in fx.z[f"shape/icm.{k}"]), k
    params = list(m.parameters())
    assert len(params) == (25 if fx.on else 19) and [p.requires_grad for p in params] == [False] * 7 + [True] * (len(params) - 7)
    assert list(D.shapes(fx.cfg)) == [k for k, p in m.named_parameters() if p.requires_grad]
    torch.manual_seed(3)
    lins = [torch.nn.Linear(i, o) for o, i in [s for k, s in D.shapes(fx.cfg).items() if k.endswith("weight") and not k.startswith("bn")]]
    for lin, k in zip(lins, ("fc1", "fc2", "forward_fc1", "forward_fc2", "inverse_fc1", "inverse_fc2")):
        assert torch.equal(lin.weight, sd[k + ".weight"]) and torch.equal(lin.bias, sd[k + ".bias"]), k
    assert float(sd["rms_obs.count"]) == np.float32(1e-4) and float(sd["rms_ri.count"]) == np.float32(1e-4)


def test_filter_worked_example_and_moments():
    """Filter gamma 0.9, three workers, four steps, r = 0 .. 11 laid out 3 x 4: the reference's stack holds four rows of [5.61, 19.366, 33.122]."""
    st = D.aliased_stack(np.zeros(3), np.arange(12.0).reshape(3, 4), 0.9)
    assert st.shape == (4, 3) and np.allclose(st.numpy(), np.tile([5.61, 19.366, 33.122], (4, 1)), rtol=0, atol=1e-12)
    true = D.filter_states(np.zeros(3), np.arange(12.0).reshape(3, 4), 0.9)
    assert np.allclose(true[0].numpy(), [0.0, 4.0, 8.0]) and torch.equal(true[-1], st[0])
    x = np.random.RandomState(0).randn(40, 3)
    m, v, c = D.moments_merge(np.zeros(3), np.zeros(3), 1e-4, x)
    assert np.allclose(m.numpy(), x.mean(0), atol=1e-5) and np.allclose(v.numpy(), x.var(0, ddof=1), rtol=1e-4) and float(c) == pytest.approx(40.0001)


def _truth_chain(fx, k, start, opt_state, dtype=torch.float64):
    """The truth over learn k from `start` (weights + block): the pre-pass, then every minibatch with its own Adam."""
    cfg, z = fx.cfg, fx.z
    cols = fx.cols(k)
    names = list(D.shapes(cfg))
    P = {n: torch.nn.Parameter(torch.as_tensor(np.asarray(start[n])).to(dtype)) for n in names}
    blk = {n: np.asarray(start[n]) if n in start else D.fresh_block(cfg)[n] for n in D.BLOCK_KEYS}
    opt = torch.optim.Adam(list(P.values()), lr=fx.lr)
    if opt_state is not None:
        opt.load_state_dict(opt_state)
    pre = D.reward_pass(cfg, {n: p.detach() for n, p in P.items()}, blk, cols["state"], cols["action"], cols["next_state"], cols["reward"], dtype=dtype)
    blk = {n: np.asarray(v.detach().double()) for n, v in pre["block"].items()}
    mbs = []
    for i in range(fx.n_minibatch()):
        idx = z[f"l{k}/mb{i}/idx"]
        u = D.update(cfg, {n: p.detach() for n, p in P.items()}, blk, cols["state"][idx], cols["action"][idx], cols["next_state"][idx], float(z["hyper/beta"]),
                     float(z["hyper/clip_grad_norm"]), dtype)
        for n, p in P.items():
            p.grad = u["clipped"][n].reshape(p.shape).clone()
        opt.step()
        for n, v in u["run"].items():
            blk[n] = np.asarray(v.detach().double())
        mbs.append(u)
    end = {n: p.detach().double().numpy() for n, p in P.items()}
    end.update(blk)
    return pre, mbs, end, opt.state_dict()


@pytest.mark.parametrize("name", D.FIXTURES)
def test_truth_reproduces_every_record_at_half_of_what_the_gpu_test_allows(name):
    """tests/icm_truth.py in float64, chained over every learn of the fixture, against the unmodified reference's records at HALF the GPU test's
    bounds: raw and normalised r_i, the stacked rewems, the mixed reward (0.5e-5 of the largest entry); every minibatch's l_f / l_i (0.5e-5
    relative); the inputs of each batch norm and the gradients raw and clipped of the first and the last minibatch (0.5 * bound("grad") of the
    segment's largest entry; the thinned records walk every segment); the block after the learn (rtol 0.5e-5, atol 0.5e-6); the end weights
    (0.25 % further than 2e-5, the worst within 1.05 lr).  The aliasing condition is re-asserted from the file."""
    fx = D.load_fixture(name)
    z, cfg = fx.z, fx.cfg
    start, opt_state = dict(fx.icm0), None
    for k in range(fx.learns):
        pre, mbs, end, opt_state = _truth_chain(fx, k, start, opt_state)
        stack = z[f"l{k}/stack"]
        assert stack.shape == (fx.T, fx.W) and all(np.array_equal(stack[0], stack[t]) for t in range(fx.T)), "the recorded stack has T equal rows"
        blk0 = fx.sub(f"l{k}/blk0/")
        true = D.filter_states(blk0["rff.rewems"], z[f"l{k}/r_raw"].reshape(fx.W, fx.T), cfg["gamma"], torch.float32)
        _, v_true, _ = D.moments_merge(blk0["rms_ri.mean"], blk0["rms_ri.var"], blk0["rms_ri.count"], true.reshape(-1, 1), torch.float32)
        v_rec = float(np.asarray(z[f"l{k}/icm1/rms_ri.var"]).reshape(-1)[0])
        assert abs(float(v_true) - v_rec) > 1e-3 * abs(v_rec), "the aliasing is visible in the fixture"
        for ours, key in ((pre["r_raw"], "r_raw"), (pre["stack"], "stack"), (pre["r_i"], "r_i"), (pre["reward"], "pre/reward")):
            margins.leq(D.rel(z[f"l{k}/{key}"], ours), 0.5e-5, f"{name} l{k} {key}: reference vs float64, / max")
        last = len(mbs) - 1
        for i, u in enumerate(mbs):
            for key in ("l_f", "l_i"):
                margins.leq(abs(float(z[f"l{k}/mb{i}/{key}"]) - float(u[key])) / abs(float(u[key])), 0.5e-5, f"{name} l{k} mb{i} {key}")
            if i in (0, last):
                if fx.on:
                    # fc1.bias has a zero exact gradient (it sits in front of bn1 and bn1_next) and random-walks under Adam: behind the first step of the first learn
                    # only bn2's input is well conditioned
                    for bn, act in (("bn1", "z1"), ("bn2", "z2"), ("bn1_next", "z1n")) if (k, i) == (0, 0) else (("bn2", "z2"),):
                        margins.leq(D.rel(z[f"l{k}/mb{i}/bn_in/{bn}"], fx.thin(u["acts"][act].numpy())), 0.5e-5, f"{name} l{k} mb{i} input of {bn}: reference vs float64, / max")
                thin = lambda g: {n: fx.thin(v.numpy()) for n, v in g.items()}
                for tag, g in (("grad_raw", thin(u["grads"])), ("grad_clip", thin(u["clipped"]))):
                    rec = fx.sub(f"l{k}/mb{i}/{tag}/")
                    for n, e in D.grad_errors(cfg, rec, g).items():
                        margins.leq(e, 0.5 * D.bound("grad"), f"{name} l{k} mb{i} {tag} {n}: reference vs float64, / max")
        ref1 = fx.sub(f"l{k}/icm1/")
        for n in D.BLOCK_KEYS:
            if n in ref1:
                atol = 1.05 * fx.lr if n in ("bn1.running_mean", "bn1_next.running_mean") else 0.5e-6  # they carry fc1.bias: the weights' cap
                np.testing.assert_allclose(ref1[n].reshape(-1), fx.thin(end[n]).reshape(-1), rtol=0.5e-5, atol=atol, err_msg=f"{name} l{k} block {n}")
        frac, worst = D.weight_caps(fx, {n: end[n] for n in D.shapes(cfg)}, ref1, {n: np.prod(sh) for n, sh in D.shapes(cfg).items()})
        margins.leq(frac, 0.0025, f"{name} l{k}: fraction of the truth's end weights further than 2e-5 from the reference's")
        margins.leq(worst, 1.05, f"{name} l{k}: the truth's worst end weight / lr")
        assert int(z[f"l{k}/icm_opt1/step"]) == (k + 1) * fx.n_minibatch()
        start = end


def test_comparator_errors_are_the_recorded_ones():
    """The float32 comparator (the reference's arithmetic: torch on the CPU in float32) against float64 on the GPU test's very inputs: every class's
    largest error is what icm_truth.E_REF records (within a quarter: torch's CPU kernels round differently from one build or thread count to the
    next), and the classes the 1e-5 convention covers stay within half of it."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        worst = _comparator_errors()
    finally:
        torch.set_num_threads(threads)
    print("float32 comparator, largest errors:", worst)
    for k, e in worst.items():
        margins.leq(e, 1.25 * D.E_REF[k], f"float32 comparator's {k} error vs the recorded {D.E_REF[k]:.3g}")
        assert e >= 0.5 * D.E_REF[k], f"{k}: the recorded {D.E_REF[k]:.3g} is more than twice the measured {e:.3g}"
    for k in ("loss", "r_i", "block"):
        assert D.E_REF[k] <= 0.5e-5 and D.bound(k) == 1e-5
    assert D.bound("grad_b2") == 4 * D.E_REF["grad_b2"] and D.bound("grad_b3") == 4 * D.E_REF["grad_b3"]


def _comparator_errors():
    worst = {k: 0.0 for k in D.E_REF}
    for tag, cfg, b in D.cases():
        w, blk, s, a, s2, idx = D.update_case(tag, cfg, b)
        u64, u32 = (D.update(cfg, w, blk, s[idx], a[idx], s2[idx], 0.2, None, dt) for dt in (torch.float64, torch.float32))
        worst["loss"] = max([worst["loss"]] + [abs(float(u32[k]) - float(u64[k])) / abs(float(u64[k])) for k in ("l_f", "l_i")])
        g = D.grad_class(cfg, b)
        worst[g] = max(worst[g], max(D.grad_errors(cfg, u32["grads"], u64["grads"]).values()))
        if cfg["bn"]:
            worst["block"] = max([worst["block"]] + [D.rel(u32["run"][k], u64["run"][k]) for k in u64["run"]])
    for tag, cfg, M in D.reward_cases():
        w, blk, s, a, s2, r = D.case_inputs(tag, cfg, M)
        o64, o32 = (D.reward_pass(cfg, w, blk, s, a, s2, r, dtype=dt) for dt in (torch.float64, torch.float32))
        worst["r_i"] = max([worst["r_i"]] + [D.rel(o32[k], o64[k]) for k in ("r_raw", "r_i", "reward")])
        worst["block"] = max([worst["block"]] + [D.rel(o32["block"][k], o64["block"][k]) for k in D.BLOCK_KEYS])
    return worst
