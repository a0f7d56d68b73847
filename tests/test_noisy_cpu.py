"""CPU-side checks of the Noisy / Dueling feature: the agents and the container are registered under the reference's keys and fail loudly
without a GPU, the C ABI carries the new entries, the parameter counts of the noisy kinds are the padded sums written out from
network/noisy.py, the container and ops.RainbowNet(kind="noisy")'s key table match a torch module written out here from noisy.py and
utils.py:89-107, and the float64 mirror of tests/mirror/noisy.py reproduces the reference's own forwards recorded in the fixtures
(tools/gen_golden_noisy.py) from the regenerated draws."""
import os
import re

import numpy as np
import pytest
import torch

from tests.util import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("jh_rbnet_learn_forward_n", "jh_rbnet_sig_abs_mean")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g

    g.build()
    from jorldy_amd import _lib

    return _lib.load()


def test_agents_and_container_are_registered_and_fail_loudly_without_a_gpu(lib):
    from jorldy_amd.core.agent import Agent, Dueling, Noisy, agent_dict
    from jorldy_amd.core.agent.dqn import DQN
    from jorldy_amd.core.network import Noisy as NoisyContainer
    from jorldy_amd.core.network import network_dict

    assert agent_dict["noisy"] is Noisy and agent_dict["dueling"] is Dueling and issubclass(Noisy, DQN) and issubclass(Dueling, DQN)
    assert network_dict["noisy"] is NoisyContainer
    if not torch.cuda.is_available():
        for name in ("noisy", "dueling"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                Agent(name, state_size=4, action_size=2)


def test_header_library_and_binding_table_carry_the_new_entries(lib):
    from jorldy_amd import _lib

    src = open(os.path.join(ROOT, "include", "jorldy_hip.h")).read()
    assert "network/noisy.py" in src and "utils.py:55-107" in src and "kind 4" in src and "kind 5" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", src), f"{name} not declared in include/jorldy_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.exported_names(), f"{name} missing from the binding table"
    assert lib.jh_abi_version() == 2


def test_param_counts_of_the_noisy_kinds_are_the_padded_sums(lib):
    """network/noisy.py:15-20: head, then (mu_w1, sig_w1) [F][H], (mu_b1, sig_b1) [H], (mu_w2, sig_w2) [H][A], (mu_b2, sig_b2) [A]; no `l`, no
    value stream; every tensor padded up to 4 floats."""
    up4 = lambda x: (x + 3) // 4 * 4
    total = lambda shapes: sum(up4(r * c) for r, c in shapes)
    lin = lambda out, inp: [(out, inp), (1, out)]
    S, H, A = 3, 8, 2
    noisy = lambda head, F: head + 2 * lin(H, F) + 2 * lin(A, H)
    for kind in (4, 5):
        assert lib.jh_rbnet_param_count_for(kind, 0, S, 0, 0, H, A, 1) == total(noisy(lin(H, S), H)), kind
        cnn = lin(32, 1 * 8 * 8) + lin(64, 32 * 4 * 4) + lin(64, 64 * 3 * 3)  # 1 x 36 x 36 -> 8 x 8 -> 3 x 3 -> 1 x 1 x 64 features
        assert lib.jh_rbnet_param_count_for(kind, 1, 1, 36, 36, H, A, 1) == total(noisy(cnn, 64)), kind
        assert lib.jh_rbnet_param_count_for(kind, 0, S, 0, 0, H, A, 3) == -1, "the noisy network has one output per action"
    assert 2 * up4(A * H) + 2 * up4(A) > 2 * A * H + 2 * A, "the case pads"
    # kinds 0-3 return what they did (tests/test_abi_cpu.py writes them out); nothing past 5
    assert lib.jh_rbnet_param_count_for(0, 0, S, 0, 0, H, A, 3) == total(lin(H, S) + lin(H, H) + 2 * lin(2 * H, H) + 2 * lin(A * 3, H) + 2 * lin(3, H))
    assert lib.jh_rbnet_param_count_for(3, 0, S, 0, 0, H, A, 3) == lib.jh_rbnet_param_count_for(0, 0, S, 0, 0, H, A, 3)
    assert lib.jh_rbnet_param_count_for(1, 0, S, 0, 0, H, A, 1) == total(lin(H, S) + lin(2 * H, H) + lin(A, H) + lin(1, H))
    assert lib.jh_rbnet_param_count_for(2, 0, S, 0, 0, H, A, 1) == total(lin(H, S) + lin(H, H) + lin(A, H))
    assert lib.jh_rbnet_param_count_for(6, 0, S, 0, 0, H, A, 1) == -1


class _RefNoisy(torch.nn.Module):
    """network/noisy.py:8-20 on head.py's mlp / cnn head with utils.py:89-107's init_weights, written out: the parameter registration order
    (head first as a sub-module -> state_dict lists the module's OWN parameters first, then head.*) and the generator's draw order."""

    def __init__(self, D_in, D_out, noise_type, D_hidden, head):
        super().__init__()
        if head == "mlp":
            self.head = torch.nn.Module()
            self.head.l = torch.nn.Linear(D_in, D_hidden)
            layers, F = [self.head.l], D_hidden
        else:
            self.head = torch.nn.Module()
            self.head.conv1 = torch.nn.Conv2d(D_in[0], 32, kernel_size=8, stride=4)
            self.head.conv2 = torch.nn.Conv2d(32, 64, kernel_size=4, stride=2)
            self.head.conv3 = torch.nn.Conv2d(64, 64, kernel_size=3, stride=1)
            d = [((v - 8) // 4 + 1) for v in D_in[1:]]
            d = [((v - 4) // 2 + 1) - 2 for v in d]
            layers, F = [self.head.conv1, self.head.conv2, self.head.conv3], 64 * d[0] * d[1]
        for l in layers:
            torch.nn.init.orthogonal_(l.weight.data, torch.nn.init.calculate_gain("relu"))
            torch.nn.init.zeros_(l.bias.data)
        for i, shape in ((1, (F, D_hidden)), (2, (D_hidden, D_out))):
            mu_init, sig_init = (1.0 / shape[0] ** 0.5, 0.5 / shape[0] ** 0.5) if noise_type == "factorized" else ((3.0 / shape[0]) ** 0.5, 0.017)
            mu_w, sig_w = torch.nn.Parameter(torch.empty(shape)), torch.nn.Parameter(torch.empty(shape))
            mu_b, sig_b = torch.nn.Parameter(torch.empty(shape[1])), torch.nn.Parameter(torch.empty(shape[1]))
            for name, p in (("mu_w", mu_w), ("sig_w", sig_w), ("mu_b", mu_b), ("sig_b", sig_b)):
                setattr(self, f"{name}{i}", p)
            mu_w.data.uniform_(-mu_init, mu_init)
            mu_b.data.uniform_(-mu_init, mu_init)
            sig_w.data.uniform_(sig_init, sig_init)
            sig_b.data.uniform_(sig_init, sig_init)
            self.bounds = getattr(self, "bounds", {})
            self.bounds[i] = (mu_init, sig_init)


CONTAINER_CASES = [("mlp", 5, 3, 32), ("cnn", (4, 44, 52), 6, 32)]


@pytest.mark.parametrize("noise_type", ["factorized", "independent"])
@pytest.mark.parametrize("head,S,A,H", CONTAINER_CASES)
def test_container_matches_the_reference_module_under_one_seed(head, S, A, H, noise_type):
    from jorldy_amd.core.network import Network

    torch.manual_seed(11)
    ref = _RefNoisy(S, A, noise_type, H, head)
    tail_ref = torch.rand(3)
    torch.manual_seed(11)
    ours = Network("noisy", S, A, noise_type, D_hidden=H, head=head)
    tail = torch.rand(3)
    assert torch.equal(tail, tail_ref), "the container leaves torch's generator where the reference's constructor does"
    sd, sd_ref = ours.state_dict(), ref.state_dict()
    assert list(sd) == list(sd_ref)
    assert list(sd)[:8] == ["mu_w1", "sig_w1", "mu_b1", "sig_b1", "mu_w2", "sig_w2", "mu_b2", "sig_b2"] and all(k.startswith("head.") for k in list(sd)[8:])
    for k, v in sd_ref.items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k
    F = 64 * 2 * 3 if head == "cnn" else H
    assert tuple(sd["mu_w1"].shape) == (F, H) and tuple(sd["mu_w2"].shape) == (H, A)
    for i in (1, 2):
        mu_init, sig_init = ref.bounds[i]
        assert float(sd[f"mu_w{i}"].abs().max()) <= mu_init and float(sd[f"mu_w{i}"].abs().max()) > 0.8 * mu_init
        assert float(sd[f"mu_b{i}"].abs().max()) <= mu_init
        for k in (f"sig_w{i}", f"sig_b{i}"):
            assert float(sd[k].min()) == float(sd[k].max()) == float(torch.tensor(sig_init, dtype=torch.float32)), k
    with pytest.raises(RuntimeError, match="parameter container"):
        ours(torch.zeros(1, 5))


def _stub_net(head, S, H, A):
    """ops.RainbowNet(kind="noisy")'s key table alone: no device, no library."""
    from jorldy_amd import ops

    class _Net(ops.RainbowNet):
        def __init__(self):
            self.kind, self.cnn, self.H, self.A = "noisy", head == "cnn", H, A
            up4 = lambda n: (n + 3) // 4 * 4
            if self.cnn:
                self.Cin = S[0]
                self.d3 = tuple((((v - 8) // 4 + 1) - 4) // 2 + 1 - 2 for v in S[1:])
                F = 64 * self.d3[0] * self.d3[1]
                segs = [("w1", 32, S[0] * 64), ("b1", 1, 32), ("w2", 64, 512), ("b2", 1, 64), ("w3", 64, 576), ("b3", 1, 64)]
            else:
                F = H
                segs = [("w1", H, S), ("b1", 1, H)]
            segs += [("mu_av1", H, F), ("sig_av1", H, F), ("mub_av1", 1, H), ("sigb_av1", 1, H), ("mu_a2", A, H), ("sig_a2", A, H), ("mub_a2", 1, A), ("sigb_a2", 1, A)]
            self.seg, off = {}, 0
            for name, rows, cols in segs:
                self.seg[name] = (off, rows, cols)
                off += up4(rows * cols)
            self.n = off
            self.device = torch.device("cpu")

        def __del__(self):
            pass

    return _Net()


@pytest.mark.parametrize("head,S,A,H", CONTAINER_CASES)
def test_key_table_round_trips_through_the_reference_state_dict(head, S, A, H):
    torch.manual_seed(5)
    ref = _RefNoisy(S, A, "factorized", H, head)
    with torch.no_grad():
        for p in ref.parameters():
            p.add_(0.1 * torch.randn_like(p))
    net = _stub_net(head, S, H, A)
    bucket = torch.zeros(net.n)
    net.import_state(ref.state_dict(), bucket)
    back = net.export_state(bucket)
    assert list(back) == list(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert back[k].shape == v.shape and torch.equal(back[k], v), k
    # the stored form: [out][in], and on the cnn head the input side ordered (y, x, c) where the reference's features are (c, y, x)
    off, rows, cols = net.seg["mu_av1"]
    stored = bucket[off : off + rows * cols].view(rows, cols)
    w = ref.state_dict()["mu_w1"]  # [F][H]
    if head == "cnn":
        y, x, c, n = 1, 2, 37, 5
        assert stored[n, (y * net.d3[1] + x) * 64 + c] == w[c * net.d3[0] * net.d3[1] + y * net.d3[1] + x, n]
    else:
        assert torch.equal(stored, w.t())
    off, rows, cols = net.seg["mu_a2"]
    assert torch.equal(bucket[off : off + rows * cols].view(rows, cols), ref.state_dict()["mu_w2"].t())


def regenerate_draws(z, F, H, A):
    """The NoisyNet draws of the fixture's learn() from its torch seed, in the reference's order (utils.py:58-60 / 75-76): network(state) layer 1, layer 2,
    then target_network(next_state) -> [{"l1": (..), "l2": (..)}] * 2 in NativeNet.pack_noise's / the mirror's format."""
    torch.manual_seed(int(z["hyper/torch_seed"]))
    independent = str(z["hyper/noise_type"]) == "independent"
    out = []
    for _ in range(2):
        d = {}
        for tag, (i, o) in (("l1", (F, H)), ("l2", (H, A))):
            d[tag] = (torch.randn(i, o), torch.randn(o)) if independent else (torch.randn(i), torch.randn(o))
        out.append(d)
    return out


@pytest.mark.parametrize("name", ["noisy", "noisy_odd"])
def test_mirror_reproduces_the_reference_forwards_of_the_fixture(name):
    """Pins tests/mirror/noisy.py (the comparator of the GPU parity tests) and the draw order to the reference's own learn()."""
    from mirror.noisy import Noisy

    z = load(name)
    S, A, H = int(z["hyper/S"]), int(z["hyper/A"]), int(z["hyper/H"])
    nets = []
    for prefix in ("sd0/", "sdt/"):
        m = Noisy(S, A, str(z["hyper/noise_type"]), D_hidden=H, head="mlp")
        m.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)})
        nets.append(m)
    draws = regenerate_draws(z, H, H, A)
    with torch.no_grad():
        q_all = nets[0](torch.from_numpy(z["learn/state"]), True, draws[0])
        next_q = nets[1](torch.from_numpy(z["learn/next_state"]), True, draws[1])
        q_mu = nets[0](torch.from_numpy(z["learn/state"]), False)
        s1, s2 = nets[0].get_sig_w_mean()
    np.testing.assert_allclose(q_all.numpy(), z["learn/q_all"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(next_q.numpy(), z["learn/next_q"], rtol=1e-5, atol=1e-6)
    assert float((q_mu - q_all).abs().max()) > 1e-3, "the draws matter"
    assert abs(float(s1) - float(z["result/sig_w1"])) < 1e-3 and abs(float(s2) - float(z["result/sig_w2"])) < 1e-3  # (the result is after one Adam step of 1e-3)


def test_fixtures_have_the_shapes_the_gpu_tests_rely_on():
    for name, (S, A, H, B, nt, head) in {"noisy": (4, 3, 32, 32, "factorized", "mlp"), "noisy_odd": (4, 5, 64, 7, "independent", "mlp"),
                                         "noisy_cnn": ((4, 44, 52), 6, 32, 8, "factorized", "cnn")}.items():
        z = load(name)
        assert (int(z["hyper/A"]), int(z["hyper/H"]), int(z["hyper/B"]), str(z["hyper/noise_type"]), str(z["hyper/head"])) == (A, H, B, nt, head)
        assert tuple(np.atleast_1d(z["hyper/S"]).tolist()) == (S if isinstance(S, tuple) else (S,))
        assert {k[7:] for k in z.files if k.startswith("result/")} == {"loss", "max_Q", "sig_w1", "sig_w2"}
        assert z["learn/q_all"].shape == (B, A) and z["learn/next_q"].shape == (B, A) and z["learn/d_q_all"].shape == (B, A)
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) <= 1 << 20
        if head == "cnn":
            assert z["buf_state"].dtype == np.uint8 and "recipe_seed" in z.files and any(k.startswith("grad_thin/") for k in z.files)
        else:
            online, target = z["sd0/mu_w1"], z["sdt/mu_w1"]
            assert not np.array_equal(online, target), "online != target"
