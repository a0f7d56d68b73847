"""core/agent/optim_state.py against torch.optim itself: what the codec reads out of a real optimizer and fills into a shadow over clones is
the same optimizer -- same state_dict, same next step.  torch only, no GPU."""
import pytest
import torch

from jorldy_amd.core.agent import optim_state
from jorldy_amd.core.optimizer import Optimizer

CONFIGS = {"adam": {"name": "adam", "lr": 3e-3, "betas": (0.8, 0.95), "eps": 1e-6},
           "rmsprop": {"name": "rmsprop", "lr": 2e-3, "alpha": 0.9, "eps": 1e-5},
           "rmsprop_centered": {"name": "rmsprop", "lr": 2e-3, "alpha": 0.9, "eps": 1e-5, "centered": True}}


def _loss(params, k):
    """Touches the first two parameters only: the third never receives a gradient."""
    return (params[0] ** 2).sum() * (k + 1) + (params[0].sum(0) * params[1][:2]).sum() + (params[1] - 0.5).pow(2).sum()


def _step(opt, params, k):
    opt.zero_grad()
    _loss(params, k).backward()
    opt.step()


def _assert_same_state_dict(a, b):
    assert list(a) == list(b) == ["state", "param_groups"] and a["param_groups"] == b["param_groups"]
    assert list(a["state"]) == list(b["state"])
    for i in a["state"]:
        assert list(a["state"][i]) == list(b["state"][i]), i
        for k, t in a["state"][i].items():
            u = b["state"][i][k]
            assert t.dtype == u.dtype and t.shape == u.shape and torch.equal(t, u), (i, k)


@pytest.fixture(params=sorted(CONFIGS))
def trained(request):
    """(config, real optimizer after three steps at a decayed lr, its parameters)."""
    cfg = CONFIGS[request.param]
    g = torch.Generator().manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(shape, generator=g)) for shape in ((3, 2), (3,), (4,))]
    opt = Optimizer(**cfg, params=params)
    for grp in opt.param_groups:
        grp["lr"] = 0.5 * cfg["lr"]
    for k in range(3):
        _step(opt, params, k)
    return cfg, opt, params


def test_read_shadow_fill_rebuilds_the_optimizer(trained):
    cfg, opt, params = trained
    steps, m, v = optim_state.read(opt, params)
    assert steps == 3 and v[2] is None and m[2] is None and v[0] is not None and v[1] is not None
    assert all(t is None for t in m) == (cfg["name"] == "rmsprop" and not cfg.get("centered", False))
    shadow, clones = optim_state.shadow(cfg, [p.detach().clone() for p in params], 0.5 * cfg["lr"])
    optim_state.fill(shadow, clones, steps, [None if t is None else t.clone() for t in m], [None if t is None else t.clone() for t in v])
    assert clones[2] not in shadow.state and 2 not in shadow.state_dict()["state"]
    _assert_same_state_dict(shadow.state_dict(), opt.state_dict())
    _step(opt, params, 3)
    _step(shadow, clones, 3)
    for p, q in zip(params, clones):
        assert torch.equal(p, q)
    _assert_same_state_dict(shadow.state_dict(), opt.state_dict())


def test_none_removes_an_entry_and_dense_zeroes_it(trained):
    cfg, opt, params = trained
    steps, m, v = optim_state.read(opt, params)
    m[0] = v[0] = None
    optim_state.fill(opt, params, steps, m, v)
    assert params[0] not in opt.state and list(opt.state_dict()["state"]) == [1]
    steps2, m2, v2 = optim_state.read(opt, params)
    assert steps2 == 3 and v2[0] is None and v2[2] is None and torch.equal(v2[1], v[1])
    for moments in (m2, v2):
        full = optim_state.dense(moments, params)
        assert [tuple(t.shape) for t in full] == [(3, 2), (3,), (4,)] and not full[0].any() and not full[2].any()
        assert full[1] is moments[1] or not full[1].any()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fresh_optimizer_reads_as_step_zero_and_no_state(name):
    opt, params = optim_state.shadow(CONFIGS[name], [torch.zeros(3, 2), torch.zeros(3)], 1e-3)
    assert optim_state.read(opt, params) == (0, [None, None], [None, None])
    assert opt.state_dict()["state"] == {} and opt.param_groups[0]["lr"] == 1e-3


def test_hyper_of_a_group():
    opt, _ = optim_state.shadow(CONFIGS["adam"], [torch.zeros(1)], 1e-4)
    assert optim_state.hyper(opt.param_groups[0]) == (1e-4, 0.8, 0.95, 1e-6, False)
    opt, _ = optim_state.shadow(CONFIGS["rmsprop_centered"], [torch.zeros(1)], 1e-4)
    assert optim_state.hyper(opt.param_groups[0]) == (1e-4, 0.9, 0.0, 1e-5, True)
    assert optim_state.hyper(opt.defaults)[0] == 2e-3
