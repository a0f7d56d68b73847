"""Float64 numpy statement of the contract of jh_reinforce_returns, jh_reinforce_loss_discrete and jh_reinforce_loss_continuous
(include/jorldy_hip.h; core/agent/reinforce.py:83-113 with network/policy.py:49-55): the comparator of tests/test_reinforce_cpu.py and
tests/test_reinforce_gpu.py (test infrastructure, not the product).  Inputs are float32 arrays; everything after them is float64.

  returns            the discounted scan over ALL rows and the population standardisation
  loss_discrete      -mean_t(log_softmax(logits)[t, a_t] ret[t]) and d(loss)/d(logits)
  loss_continuous    -mean over T * A of Normal(clamp(mu_raw, -5, 5), exp(tanh(log_std_raw))).log_prob(atanh(clamp(action))) ret[t] and d(loss)/d(raw head)
  loss_torch         the same two the way the reference writes them (log of a gathered softmax, torch's Normal) with autograd in a given dtype:
                     float32 is the comparator whose own error the acceptance rule of the GPU tests needs, float64 cross-checks the numpy statement
and the case builders of the kernel sweeps, the reader of the fixtures of tools/gen_golden_reinforce.py and the curve configuration."""
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("reinforce_discrete", "reinforce_continuous", "reinforce_nostd", "reinforce_cartpole")
COLUMNS = ("state", "action", "reward", "next_state", "done")
MAX_ROWS = 65536
# float32(-1 + 1e-7) and float32(1 - 1e-7): the reference clamps the float32 action tensor (see the note in tests/fp64_truth.py, ppo_head_grads_float64)
CLAMP_HI = float(np.float32(1 - 1e-7))
assert CLAMP_HI == 1.0 - 2.0 ** -23 and float(np.float32(-1 + 1e-7)) == -CLAMP_HI

# ---- the kernel sweeps.  The scan: one workgroup of 1024 threads, thread i owns per = ceil(T / 1024) consecutive rows, ceil(T / per) chunks in
# whole waves of 64.  The issue's sizes, then both sides of every boundary of that dispatch: one wave | two (64 | 65 chunks; 128 | 129), the last
# size with one row per thread | the first with two (1024 | 1025: 16 waves of 1-row chunks | 513 chunks in 9 waves), two rows | three (2048 | 2049),
# a chunk count that leaves the last wave ragged and the last chunk short (4097: per 5, 820 chunks, the last of 2 rows), 63 | 64 rows per thread
# (64512 | 64513) and the cap.
RETURN_T = (1, 2, 63, 64, 65, 1023, 1024, 1025, 65536, 128, 129, 2048, 2049, 4097, 64512, 64513, 65535)
RETURN_GAMMA = (0.99, 1.0, 0.5)
# the losses: 256 rows per workgroup, at most 64 workgroups, grid-stride beyond (more than 16384 rows): one row, less than a wave, a wave | a wave
# and a row, several workgroups with a ragged last one (1025, 4097), and both sides of the grid-stride threshold (16384 | 16385)
LOSS_T = (1, 5, 64, 65, 1025, 4097, 16384, 16385)
LOSS_A = {"discrete": (2, 3, 18, 64), "continuous": (1, 3, 17, 32)}
# the reference on the oracle's CartPole (tools/gen_golden_reinforce.py --only curves): config.reinforce.cartpole with the learning rate and the
# budget the issue starts the search at (lr 1e-3, 20000 steps; see the JSON's `search` for what the reference did at each budget tried)
CURVE_CONFIG = dict(steps=20000, seeds=(1, 2, 3), run_step=20000, chunk=1000,
                    agent=dict(state_size=4, action_size=2, hidden_size=512, network="discrete_policy", head="mlp", optim_config={"name": "adam", "lr": 1e-3}, gamma=0.99,
                               use_standardization=True, lr_decay=True))


# ---------------------------------------------------------------------------------------------- the truth
def scan(reward, gamma):
    """ret[t] = reward[t] + gamma ret[t + 1] over all rows, float64."""
    ret = np.asarray(reward, dtype=np.float64).reshape(-1).copy()
    acc = 0.0
    g = float(gamma)
    for t in range(ret.size - 1, -1, -1):
        acc = ret[t] + g * acc
        ret[t] = acc
    return ret


def returns(reward, gamma, standardize=True):
    ret = scan(reward, gamma)
    if standardize:
        ret = (ret - ret.mean()) / (ret.std() + 1e-7)
    return ret


def _lsm(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))


def loss_discrete(logits, action, ret):
    """logits [T, A], action [T], ret [T] -> dict(loss, grad [T, A]) in float64."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    T, A = z.shape
    a = np.clip(np.asarray(action).reshape(-1).astype(np.int64), 0, A - 1)
    r = np.asarray(ret, dtype=np.float32).astype(np.float64).reshape(-1)
    lp = _lsm(z)
    rows = np.arange(T)
    loss = float(-(lp[rows, a] * r).mean())
    onehot = np.zeros((T, A))
    onehot[rows, a] = 1.0
    return dict(loss=loss, grad=r[:, None] * (np.exp(lp) - onehot) / T, logp=lp[rows, a])


def loss_continuous(head, action, ret):
    """head [T, 2A] = [mu_raw | log_std_raw], action [T, A], ret [T] -> dict(loss, grad [T, 2A]) in float64."""
    h = np.asarray(head, dtype=np.float32).astype(np.float64)
    T, A = h.shape[0], h.shape[1] // 2
    mu_raw, ls_raw = h[:, :A], h[:, A:]
    r = np.asarray(ret, dtype=np.float32).astype(np.float64).reshape(-1, 1)
    a = np.clip(np.asarray(action, dtype=np.float32).reshape(T, A), np.float32(-1 + 1e-7), np.float32(1 - 1e-7)).astype(np.float64)
    z = np.arctanh(a)
    mu, ls = np.clip(mu_raw, -5.0, 5.0), np.tanh(ls_raw)
    var = np.exp(2.0 * ls)
    d = z - mu
    lp = -0.5 * d * d / var - ls - 0.5 * np.log(2.0 * np.pi)
    loss = float(-(lp * r).mean())
    w = r / (T * A)
    inside = (mu_raw >= -5.0) & (mu_raw <= 5.0)
    g_mu = np.where(inside, -w * d / var, 0.0)
    g_ls = -w * (d * d / var - 1.0) * (1.0 - ls * ls)
    return dict(loss=loss, grad=np.concatenate([g_mu, g_ls], 1), logp=lp)


def loss_torch(kind, head, action, ret, dtype=None):
    """reinforce.py:98-106 from the raw head on, as the reference writes it, in `dtype` with autograd -> dict(loss, grad)."""
    import torch

    dtype = dtype or torch.float32
    h = torch.as_tensor(np.asarray(head, dtype=np.float32)).to(dtype).requires_grad_(True)
    r = torch.as_tensor(np.asarray(ret, dtype=np.float32)).to(dtype).reshape(-1, 1)
    if kind == "continuous":
        A = h.shape[1] // 2
        mu, std = torch.clamp(h[:, :A], min=-5.0, max=5.0), torch.tanh(h[:, A:]).exp()
        a = torch.clamp(torch.as_tensor(np.asarray(action, dtype=np.float32)).reshape(-1, A), -1 + 1e-7, 1 - 1e-7).to(dtype)  # clamped as a float32 tensor
        log_prob = torch.distributions.Normal(mu, std).log_prob(torch.atanh(a))
    else:
        A = h.shape[1]
        pi = torch.exp(torch.log_softmax(h, dim=-1))
        a = torch.as_tensor(np.clip(np.asarray(action).reshape(-1, 1).astype(np.int64), 0, A - 1))
        log_prob = torch.log(pi.gather(1, a))
    loss = -(log_prob * r).mean()
    loss.backward()
    return dict(loss=float(loss.detach()), grad=h.grad.numpy().astype(np.float64))


# ---------------------------------------------------------------------------------------------- kernel cases
def reward_case(T, kind, seed=0):
    """float32 rewards of one episode: `cartpole` (0.1 per step, -1 at the end) or `normal` (random normal)."""
    if kind == "cartpole":
        r = np.full(T, 0.1, np.float32)
        r[-1] = -1.0
        return r
    return np.random.RandomState(1000 * seed + T).randn(T).astype(np.float32)


def return_cases():
    """(T, gamma, standardize, reward kind) of the scan sweep."""
    return [(T, g, s, k) for T in RETURN_T for g in RETURN_GAMMA for s in (True, False) for k in ("cartpole", "normal")]


def loss_case(kind, T, A, seed=0):
    """Synthetic inputs of one loss-kernel call: dict(head, action, ret).  Continuous: mu_raw has entries beyond +-5 (never within 1e-3 of the
    bound), the actions hold exact +-1 and nothing strictly between the float32 clamp bound and 1."""
    rs = np.random.RandomState(7919 * seed + 31 * T + A + (500000 if kind == "continuous" else 0))
    ret = rs.randn(T).astype(np.float32)
    if kind == "discrete":
        return dict(head=(2.0 * rs.randn(T, A)).astype(np.float32), action=rs.randint(0, A, size=T).astype(np.float32), ret=ret)
    mu = (3.0 * rs.randn(T, A)).astype(np.float32)
    near = np.abs(np.abs(mu) - 5.0) < 1e-3
    mu[near] = np.float32(4.5)
    mu.reshape(-1)[0] = np.float32(6.25)  # clamped, whatever the draw
    if mu.size > 1:
        mu.reshape(-1)[-1] = np.float32(-7.5)
    action = np.tanh(1.5 * rs.randn(T, A)).astype(np.float32)
    action[np.abs(action) > np.float32(CLAMP_HI)] = 1.0
    action.reshape(-1)[:: max(1, action.size // 3)] = 1.0  # saturated actions
    if action.size > 1:
        action.reshape(-1)[1] = -1.0
    head = np.concatenate([mu, (1.5 * rs.randn(T, A)).astype(np.float32)], 1)
    return dict(head=np.ascontiguousarray(head), action=action, ret=ret)


def case_truth(kind, c, dtype=None):
    if dtype is not None:
        return loss_torch(kind, c["head"], c["action"], c["ret"], dtype)
    return (loss_continuous if kind == "continuous" else loss_discrete)(c["head"], c["action"], c["ret"])


# ---------------------------------------------------------------------------------------------- fixtures
def thin(a, limit, stride=61):
    a = np.asarray(a)
    return a if (not limit or a.size <= limit) else np.ascontiguousarray(a.reshape(-1)[::stride])


def recipe_weights(shapes, seed, synth):
    """Recipe weights of the policy (oracle/synth.py's streams, keyed by name); the policy's last layer is scaled down as ppo_recipe scales heads."""
    sd = synth.recipe_state_dict([(f"reinforce.{k}", s) for k, s in shapes.items()], seed)
    out = OrderedDict((k[len("reinforce."):], v) for k, v in sd.items())
    for k in out:
        if k.split(".")[0] in ("pi", "mu", "log_std") and out[k].ndim == 2:
            out[k] = np.ascontiguousarray(out[k] * np.float32(0.3), dtype=np.float32)
    return out


class Fixture:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN, name + ".npz"))
        h = lambda k: self.z[f"hyper/{k}"]
        self.S, self.A, self.H = int(h("S")), int(h("A")), int(h("H"))
        self.lr, self.gamma, self.run_step = float(h("lr")), float(h("gamma")), int(h("run_step"))
        self.standardize, self.cont, self.recipe, self.thin_limit = bool(int(h("standardize"))), bool(int(h("cont"))), bool(int(h("recipe"))), int(h("thin_limit"))
        self.rows = [int(v) for v in h("rows")]
        self.learns = len(self.rows)
        self.kind = "continuous" if self.cont else "discrete"

    def thin(self, a):
        return thin(a, self.thin_limit)

    def agent_kwargs(self):
        return dict(state_size=self.S, action_size=self.A, hidden_size=self.H, network="continuous_policy" if self.cont else "discrete_policy", head="mlp",
                    optim_config={"name": "adam", "lr": self.lr}, gamma=self.gamma, use_standardization=self.standardize, run_step=self.run_step, lr_decay=True)

    def sd0(self):
        """The starting weights: stored, or (recipe fixtures) regenerated from the seed."""
        if self.recipe:
            from oracle import synth

            shapes = OrderedDict((k[len("shape/"):], tuple(int(x) for x in self.z[k])) for k in self.z.files if k.startswith("shape/"))
            return recipe_weights(shapes, int(self.z["hyper/recipe_seed"]), synth)
        return OrderedDict((k[len("sd0/"):], self.z[k]) for k in self.z.files if k.startswith("sd0/"))

    def learn(self, k):
        p = f"l{k}/"
        return {key[len(p):]: self.z[key] for key in self.z.files if key.startswith(p)}

    def transitions(self, k):
        """The stored rows of learn k as the list of one-row transitions the single-mode loop hands to process(), with their step numbers."""
        rec = self.learn(k)
        T = self.rows[k]
        trs = [{c: rec[f"in/{c}"][t : t + 1] for c in COLUMNS} for t in range(T)]
        return trs, [int(s) for s in rec["steps"]]


def load_fixture(name):
    return Fixture(name)


def curve_tenths(curve):
    """(mean of the first tenth, mean of the last tenth) of a curve of per-chunk means."""
    n = max(1, len(curve) // 10)
    return float(np.mean(curve[:n])), float(np.mean(curve[-n:]))
