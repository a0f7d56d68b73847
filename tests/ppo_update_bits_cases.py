"""The calls behind tests/golden/ppo_update_bits.npz: what tools/gen_ppo_update_bits.py records and tests/test_ppo_update_bits_gpu.py replays.

Every record is a sequence of PPONet.ppo_update calls from seeded inputs on a seeded network, and holds the state the sequence leaves behind:
parameters, gradient bucket, exp_avg, exp_avg_sq (after the last call), the statistics row and the 16 floats of the optimizer's hyper block after
every call, and a SHA-256 digest of each bucket after every call.  The fixture is a recording of the library's own results at the commit that
introduced it; a kernel change that is meant to keep the arithmetic must reproduce it bit for bit.

DISC_REG_MAX is the largest discrete action count that takes the loss kernel's register-resident row form (csrc/jh_ppo.hip: kDiscCache); one case sits
on it and one just above it."""
import hashlib
from collections import namedtuple

import numpy as np

DISC_REG_MAX = 4
LR, B1, B2, ADAM_EPS = 3e-4, 0.9, 0.999, 1e-8
EPS_CLIP, VF, ENT, MAX_NORM = 0.1, 1.0, 0.01, 0.5
CALLS = 3

Case = namedtuple("Case", "name cont S A B H indexed step digest_only")
CASES = (
    Case("disc_a2_b256", False, 4, 2, 256, 64, False, 0, False),
    Case("disc_a2_b256_step1000", False, 4, 2, 256, 64, False, 1000, False),
    Case("disc_a2_b100_idx", False, 4, 2, 100, 64, True, 0, False),
    Case("disc_cut_b250", False, 8, DISC_REG_MAX, 250, 64, False, 0, False),
    Case("disc_cut1_b250", False, 8, DISC_REG_MAX + 1, 250, 64, False, 0, False),
    Case("disc_a7_b64", False, 8, 7, 64, 64, False, 0, False),
    Case("cont_a3_b100", True, 11, 3, 100, 64, False, 0, False),
    Case("disc_a2_b256_h512", False, 4, 2, 256, 512, False, 0, True),
)
IDS = tuple(c.name for c in CASES)
BUCKETS = ("params", "grads", "m", "v")


def n_params(c):
    n_head = c.A * c.H + c.A
    return c.H * c.S + c.H + c.H * c.H + c.H + n_head * (2 if c.cont else 1) + c.H + 1


def make_inputs(c, seed=None):
    """Seeded host arrays: the rollout columns (M rows; the minibatch is the first B rows, or B rows picked through an index list), the starting
    parameters and, for a start away from step 0, moments as an optimizer in flight would hold them."""
    rng = np.random.RandomState(1234 + 7 * CASES.index(c) if seed is None else seed)
    M = c.B + 44 if c.indexed else c.B
    d = {"x": rng.randn(M, c.S).astype(np.float32)}
    d["idx"] = rng.permutation(M)[: c.B].astype(np.int64) if c.indexed else None
    if c.cont:
        act = np.tanh(rng.randn(M, c.A)).astype(np.float32)
        d["action"] = act
        z = np.arctanh(np.clip(act.astype(np.float64), -0.99999988, 0.99999988))
        d["logp_old"] = (-0.5 * z * z - 0.9189385332 + 0.05 * rng.randn(M, c.A)).astype(np.float32)
    else:
        d["action"] = rng.randint(0, c.A, size=(M, 1)).astype(np.float32)
        d["logp_old"] = (np.log(1.0 / c.A) + 0.1 * rng.randn(M, 1)).astype(np.float32)
    d["adv"] = rng.randn(M, 1).astype(np.float32)
    d["ret"] = rng.randn(M, 1).astype(np.float32)
    d["value_old"] = (d["ret"] + 0.3 * rng.randn(M, 1)).astype(np.float32)
    n = n_params(c)
    d["p0"] = (rng.randn(n) / np.sqrt(c.H)).astype(np.float32)
    d["m0"] = (1e-3 * rng.randn(n)).astype(np.float32) if c.step else np.zeros(n, np.float32)
    d["v0"] = (1e-6 * rng.rand(n)).astype(np.float32) if c.step else np.zeros(n, np.float32)
    return d


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8).copy()


def make_net(c, d):
    import torch

    from jorldy_amd import ops

    net = ops.PPONet(c.S, c.H, c.A, c.cont, ((c.B + 255) // 256 + 1) * 256, "cuda:0")
    assert net.n_params == d["p0"].size, (net.n_params, d["p0"].size)
    net.params.copy_(torch.from_numpy(d["p0"]))
    net.m.copy_(torch.from_numpy(d["m0"]))
    net.v.copy_(torch.from_numpy(d["v0"]))
    net.grads.zero_()
    net.set_hyper(LR, B1, B2, ADAM_EPS, step=float(c.step))
    return net


def to_device(d):
    import torch

    return {k: (torch.from_numpy(v).cuda() if v is not None else None) for k, v in d.items() if k in ("x", "idx", "action", "adv", "ret", "value_old", "logp_old")}


def hyper_of(net):
    from jorldy_amd import ops

    return ops._wrap_device(net.hyper_ptr(), (16,), __import__("torch").float32, net.device, owner=net)


def update(net, dev, stats, do_adam=True):
    net.ppo_update(dev["x"], dev["idx"], dev["action"], dev["adv"], dev["ret"], dev["value_old"], dev["logp_old"], EPS_CLIP, VF, ENT, MAX_NORM, stats, do_adam=do_adam)


def snapshot(net, stats):
    """-> (the four buckets, the statistics row, the hyper block) as host arrays, after a device synchronisation."""
    import torch

    torch.cuda.synchronize()
    buckets = {k: getattr(net, k).cpu().numpy().copy() for k in BUCKETS}
    return buckets, stats.cpu().numpy().copy(), hyper_of(net).cpu().numpy().copy()


class Recorder:
    """Collects the per-call rows of one record and lays the record out under `<name>/...` keys."""

    def __init__(self, name, digest_only):
        self.name, self.digest_only, self.stats, self.hyper, self.digests, self.last = name, digest_only, [], [], {k: [] for k in BUCKETS}, None

    def add(self, net, stats):
        buckets, st, hy = snapshot(net, stats)
        self.stats.append(st)
        self.hyper.append(hy)
        for k in BUCKETS:
            self.digests[k].append(digest(buckets[k]))
        self.last = buckets

    def record(self):
        out = {f"{self.name}/stats": np.stack(self.stats), f"{self.name}/hyper": np.stack(self.hyper)}
        for k in BUCKETS:
            out[f"{self.name}/sha256/{k}"] = np.stack(self.digests[k])
            if not self.digest_only:
                out[f"{self.name}/{k}"] = self.last[k]
        return out


def run_case(c, calls=CALLS):
    """CALLS consecutive ppo_update(do_adam=True) calls of case c."""
    import torch

    d = make_inputs(c)
    net, dev = make_net(c, d), to_device(d)
    rec = Recorder(c.name, c.digest_only)
    for _ in range(calls):
        stats = torch.full((8,), -1.0, device="cuda")
        update(net, dev, stats)
        rec.add(net, stats)
    return rec.record()


def run_no_adam(c=CASES[0]):
    """The data-parallel shape of the update: ppo_update(do_adam=False) leaves a complete gradient bucket, adam_step applies it."""
    import torch

    d = make_inputs(c)
    net, dev = make_net(c, d), to_device(d)
    rec = Recorder("noadam_" + c.name, False)
    for _ in range(CALLS):
        stats = torch.full((8,), -1.0, device="cuda")
        update(net, dev, stats, do_adam=False)
        net.adam_step(MAX_NORM)
        rec.add(net, stats)
    return rec.record()


def run_set_hyper(c=CASES[0], k=1000):
    """One update from step 0, then set_hyper(step=k) and a stand-alone update: the bias corrections must be those of step k + 1."""
    import torch

    d = make_inputs(c)
    net, dev = make_net(c, d), to_device(d)
    rec = Recorder("sethyper_" + c.name, False)
    stats = torch.full((8,), -1.0, device="cuda")
    update(net, dev, stats)
    rec.add(net, stats)
    net.set_hyper(LR, B1, B2, ADAM_EPS, step=float(k))
    stats = torch.full((8,), -1.0, device="cuda")
    update(net, dev, stats)
    rec.add(net, stats)
    return rec.record()


def run_all():
    out = {}
    for c in CASES:
        out.update(run_case(c))
    out.update(run_no_adam())
    out.update(run_set_hyper())
    return out
