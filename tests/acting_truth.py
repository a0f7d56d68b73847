"""The acting side of PPO against float64 (test infrastructure, not the product): which acting path a collector case reaches, a scripted
vector env whose rollout can be recomputed from the stored actions alone, the cases of tests/test_acting_truth_{cpu,gpu}.py and their policies.

  dispatch(case)    the selection rules of csrc/jh_collect.hip (collector_create) and csrc/jh_persist.hip (jh_persist_create, jh_persist_can_split,
                    jh_persist_begin) restated: -> dict(persist, lookahead, split, rows, SP, NCH, PI, RT, G, reduced), and `path`
  ScriptedVec       a deterministic Python vector env with the PythonEnvTable protocol (obs, step with optional row ranges, fork, copy_row)
  CASES             one entry per dispatch edge (by_name(name) finds one)
  policy / sharp    the reference's policy-value module (tests/mirror) in float64 with float32-representable weights, and its float32 twin
  make_env / make_model / modules_of / truths / greedy_rollout    what both test files do with a case
"""
import numpy as np
import torch

T_STEPS = 5   # timesteps per run of the tests
N_RUNS = 2    # runs per case (a learn() in between: the second run acts with updated weights)
SHARP_P = 1.0 - 1e-9   # a row is "decided" when the float64 policy puts at least this much on one action
SHARP_ROWS = 0.9       # ... and at least this share of a sharp case's rows must be decided

SWITCHES = ("JH_COLLECT_PERSISTENT", "JH_COLLECT_SPLIT", "JH_COLLECT_LOOKAHEAD", "JH_PERSIST_REDUCE", "JH_COLLECT_CAPTURE", "JH_COLLECT_TEST_STALL")


# ---------------------------------------------------------------------------------------------- which path a case reaches
def n_out_of(case):
    return (2 * case["A"] if case["cont"] else case["A"]) + 1


def _poll_instructions(granules):  # jh_persist.hip: persist_poll_instructions
    return ((granules + 1) // 2 + 63) // 64


def _can_split(rows0, rows1, S):  # jh_persist.hip: jh_persist_can_split
    return 1 <= rows0 <= 16 and 1 <= rows1 <= 16 and _poll_instructions(rows0 * S) == _poll_instructions(rows1 * S)


def dispatch(case):
    """-> dict(persist, lookahead, split, rows, SP, NCH, PI, RT, G, reduced, path).  SP .. reduced are None without the persistent kernel;
    path is "persistent", "fused" (one jh_gemm16_act_fused launch per step: n_out <= 8) or "separate" (the separate-call forward)."""
    W, S, A, H, env = case["W"], case["S"], case["A"], case["H"], case["env"]
    n_out = n_out_of(case)
    sw = lambda k: int(env[k]) if k in env else None
    mode = 1 if sw("JH_COLLECT_PERSISTENT") is None else sw("JH_COLLECT_PERSISTENT")
    # collector_create: mode 1, W <= 32, W * S <= 512 and what jh_persist_create accepts
    persist = mode == 1 and W <= 32 and W * S <= 512 and 1 <= S <= 16 and H in (64, 128, 256, 512) and n_out <= 12
    if not persist:
        return dict(persist=0, lookahead=1, split=0, rows=W, SP=None, NCH=None, PI=None, RT=None, G=None, reduced=None, path="fused" if n_out <= 8 else "separate")
    forkable = case["kind"] in ("cartpole", "scripted-fork")
    builtin = case["kind"] in ("cartpole", "control")
    lookahead = 1
    if forkable and not case["cont"] and A == 2 and 3 * W <= 32 and 3 * W * S <= 128:
        la = sw("JH_COLLECT_LOOKAHEAD")
        lookahead = 2 if la is None or la >= 2 else 1
    per_env = 3 if lookahead == 2 else 1
    half0, half1 = per_env * ((W + 1) // 2), per_env * (W - (W + 1) // 2)
    split = W >= 2 and (lookahead == 2 or builtin) and sw("JH_COLLECT_SPLIT") != 0 and _can_split(half0, half1, S)
    rows = per_env * W
    # jh_persist_begin
    win = half0 * S if split else rows * S
    reduce = sw("JH_PERSIST_REDUCE")
    return dict(persist=1, lookahead=lookahead, split=int(split), rows=rows, SP=(S + 3) // 4 * 4, NCH=H // 64, PI=_poll_instructions(win),
                RT=2 if split or rows > 16 else 1, G=(n_out + 2) // 3, reduced=int(reduce == 1) if reduce is not None else int(split and rows == 32), path="persistent")


# ---------------------------------------------------------------------------------------------- the scripted env
_U = np.uint64
_C1, _C2, _C3 = _U(0x9E3779B97F4A7C15), _U(0xBF58476D1CE4E5B9), _U(0x94D049BB133111EB)


def _mix(x):  # splitmix64's finaliser on uint64 arrays
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=np.uint64) + _C1
        x = (x ^ (x >> _U(30))) * _C2
        x = (x ^ (x >> _U(27))) * _C3
        return x ^ (x >> _U(31))


class ScriptedVec:
    """W rows; a row's state is (row id, episode number, step in the episode, 64-bit checksum of the actions taken in this episode).  Observation
    and reward are pure functions of that state and the env's seed, episodes end at scripted lengths (row id mod 3 == 0: the first episode
    ends at its step 1 and the second at its step 2, i.e. at t = 1 and t = 4 of a five-step run; == 1: at step 4), a finished row resets itself.
    Observations: float32, one value in eight an exact zero, both signs, magnitudes 1e-3 .. 8 (log-uniform).  `forkable` adds fork / copy_row,
    which is what PythonEnvTable takes as the capability to be stepped ahead on copies."""

    def __init__(self, W, S, A, cont, forkable=False, seed=0):
        self.W, self.state_size, self.action_size, self.action_type = int(W), int(S), int(A), "continuous" if cont else "discrete"
        self.cont, self.seed, self.forkable = bool(cont), int(seed), bool(forkable)
        self.rid = np.arange(W, dtype=np.int64)
        self.ep = np.zeros(W, np.int64)
        self.t = np.zeros(W, np.int64)
        self.chk = np.zeros(W, np.uint64)
        if forkable:
            self.fork = lambda rows: ScriptedVec(rows, S, A, cont, True, seed)
            self.copy_row = self._copy_row

    def _copy_row(self, di, src, si):
        self.rid[di], self.ep[di], self.t[di], self.chk[di] = src.rid[si], src.ep[si], src.t[si], src.chk[si]

    # -- pure functions of (seed, state)
    def _key(self, rid, ep, t, chk):
        with np.errstate(over="ignore"):
            k = _mix(np.full(len(rid), self.seed, np.uint64) * _C2 + rid.astype(np.uint64))
            k = _mix(k + ep.astype(np.uint64))
            k = _mix(k + t.astype(np.uint64))
        return _mix(k ^ chk)

    def _obs_of(self, rid, ep, t, chk):
        with np.errstate(over="ignore"):
            h = _mix(self._key(rid, ep, t, chk)[:, None] + (np.arange(self.state_size, dtype=np.uint64)[None, :] + _U(1)) * _C3)
        u = (h >> _U(11)).astype(np.float64) / 9007199254740992.0
        mag = 1e-3 * 8000.0 ** u
        v = np.where((h >> _U(3)) & _U(1) == 1, -mag, mag)
        return np.where(h & _U(7) == 0, 0.0, v).astype(np.float32)

    def _reward_of(self, rid, ep, t, chk):
        return (((self._key(rid, ep, t, chk) >> _U(20)) % _U(2001)).astype(np.float64) / 1000.0 - 1.0).astype(np.float32)

    def _length_of(self, rid, ep):
        with np.errstate(over="ignore"):
            hashed = 2 + (_mix(_mix(np.full(len(rid), self.seed + 77, np.uint64)) + rid.astype(np.uint64) * _C1 + ep.astype(np.uint64)) % _U(7)).astype(np.int64)  # 2 .. 8
        first = np.where(rid % 3 == 0, 2, np.where(rid % 3 == 1, 5, hashed))
        second = np.where(rid % 3 == 0, 3, hashed)
        return np.where(ep == 0, first, np.where(ep == 1, second, hashed))

    def _fold(self, chk, action):
        a = np.ascontiguousarray(action)
        if self.cont:
            bits = a.astype(np.float32).reshape(len(chk), self.action_size).view(np.uint32).astype(np.uint64)
            with np.errstate(over="ignore"):
                for k in range(self.action_size):
                    chk = _mix(chk ^ _mix(bits[:, k] + np.full(len(chk), k + 1, np.uint64) * _C2))
            return chk
        return _mix(chk ^ _mix(a.reshape(-1).astype(np.int64).astype(np.uint64)))

    # -- the VecCollector / PythonEnvTable protocol
    def obs(self, out=None, r0=0, r1=None):
        r1 = self.W if r1 is None else r1
        o = self._obs_of(self.rid[r0:r1], self.ep[r0:r1], self.t[r0:r1], self.chk[r0:r1])
        if out is None:
            return o
        out[:] = o
        return out

    def step(self, action, nxt, rew, done, r0=0, r1=None):
        """The rows r0 .. r1-1 take action [r1 - r0](, A); nxt / rew / done hold the rows of the range."""
        r1 = self.W if r1 is None else r1
        s = slice(r0, r1)
        rid, ep = self.rid[s], self.ep[s]
        t = self.t[s] + 1
        chk = self._fold(self.chk[s], action)
        nxt[:] = self._obs_of(rid, ep, t, chk)
        rew[:] = self._reward_of(rid, ep, t, chk)
        d = t >= self._length_of(rid, ep)
        done[:] = d
        self.ep[s] = np.where(d, ep + 1, ep)
        self.t[s] = np.where(d, 0, t)
        self.chk[s] = np.where(d, _U(0), chk)
        return nxt, rew, done

    def replay(self, actions):
        """Steps THIS env through actions [W, T](, A) -> (state [W, T, S], next_state [W, T, S], reward [W, T], done [W, T] bool): what an env built
        like this one and in this one's state must have produced when those actions were taken."""
        actions = np.asarray(actions)
        W, T, S = self.W, actions.shape[1], self.state_size
        st, ns = np.empty((W, T, S), np.float32), np.empty((W, T, S), np.float32)
        rw, dn = np.empty((W, T), np.float32), np.empty((W, T), np.uint8)
        for t in range(T):
            st[:, t] = self.obs()
            self.step(actions[:, t], ns[:, t], rw[:, t], dn[:, t])
        return st, ns, rw, dn.astype(bool)


# ---------------------------------------------------------------------------------------------- the cases
def _case(name, kind, W, S, A, H, cont=None, env=None, sharp=False, base=None):
    cont = (kind == "control") if cont is None else cont
    return dict(name=name, kind=kind, W=W, S=S, A=A, H=H, cont=bool(cont), env=dict(env or {}), sharp=sharp, base=base or name)


def _with(case, name, **env):
    return dict(case, name=name, env=dict(case["env"], **env), base=case["base"])


def _build_cases():
    c = []
    # persistent, default switches
    a = {(S, H): _case(f"a-S{S}-H{H}", "control", 4, S, 2, H) for S in (2, 7, 11, 16) for H in (64, 128, 256, 512)}
    c += list(a.values())
    b = _case("b", "control", 32, 11, 3, 512)
    c.append(b)
    c += [_case(f"c-W{W}", "control", W, 4, 1, 64) for W in (2, 3, 31)]
    c.append(_case("d", "control", 25, 10, 3, 128))
    e = _case("e", "scripted", 16, 5, 11, 128, cont=False)
    f = _case("f", "scripted", 17, 9, 8, 256, cont=False)
    g = _case("g", "scripted", 1, 13, 5, 512, cont=True)
    c += [e, f, g, _case("h", "scripted", 15, 3, 4, 64, cont=True)]
    i = [_case(f"i-W{W}", "scripted-fork", W, S, 2, H, cont=False) for W, S, H in ((10, 4, 64), (5, 8, 128), (2, 16, 256))]
    c += i
    c.append(_case("j", "cartpole", 10, 4, 2, 512, cont=False))
    # persistent, switches set
    c.append(_with(b, "k", JH_COLLECT_SPLIT="0"))
    c.append(_case("l", "control", 32, 16, 1, 64, env={"JH_COLLECT_SPLIT": "0"}))
    c.append(_with(i[0], "m", JH_COLLECT_SPLIT="0"))
    c += [_with(f, "n-f", JH_PERSIST_REDUCE="1"), _with(a[(7, 64)], "n-a", JH_PERSIST_REDUCE="1"), _with(i[0], "n-i", JH_PERSIST_REDUCE="1")]
    c.append(_with(b, "o", JH_PERSIST_REDUCE="0"))
    # one launch per step
    c += [_with(x, f"p-{x['name']}", JH_COLLECT_PERSISTENT="0") for x in (b, e, g)]
    c += [_case(f"q-H{H}-W{W}", "control", W, 11, 3, H) for H in (32, 96) for W in (1, 16, 17, 33)]
    c.append(_case("q-S17", "control", 5, 17, 3, 64))
    c.append(_case("q-cont13", "scripted", 5, 17, 6, 64, cont=True))
    c.append(_case("q-disc13", "scripted", 9, 6, 12, 64, cont=False))
    # beyond the list: the W1 fragments in REGISTERS (SP <= 8) under more than one poll instruction -- no case above has more than 128 granules in
    # a window at S <= 8 -- at a width that is no multiple of 4 (140 granules unsplit, two row tiles)
    c.append(_case("r", "scripted", 20, 7, 2, 128, cont=True))
    # near-deterministic discrete policies: the stored action must be the float64 argmax
    c.append(dict(e, name="e-sharp", sharp=True))
    c.append(dict(i[0], name="i-sharp", sharp=True))
    return c


CASES = _build_cases()


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def case_seed(case):
    """One integer per BASE case (a switch variant acts with its base case's weights on its base case's env)."""
    return 1000 + sum((k + 1) * ord(ch) for k, ch in enumerate(case["base"]))


def make_env(case):
    """The env the collector runs on (fresh, in its start state)."""
    W, S, A, seed = case["W"], case["S"], case["A"], case_seed(case) % 97
    if case["kind"] == "control":
        from jorldy_amd import ops

        return ops.ControlVec(W, S, A, seed=seed)
    if case["kind"] == "cartpole":
        from jorldy_amd import ops

        return ops.CartPoleVec(W, seed=seed)
    return ScriptedVec(W, S, A, case["cont"], forkable=case["kind"] == "scripted-fork", seed=seed)


class _OracleReplay:
    """`replay` for the library's own envs: the oracle's env of the same seed (bit-identical to the native one: tests/test_abi_cpu.py)."""

    def __init__(self, orc):
        self.o = orc

    def replay(self, actions):
        actions = np.asarray(actions)
        W, T = actions.shape[:2]
        st, ns, rw, dn = [], [], [], []
        for t in range(T):
            st.append(self.o.obs())
            n, r, d = self.o.step(actions[:, t])
            ns.append(n), rw.append(r), dn.append(d)
        stack = lambda xs: np.stack(xs, 1)
        return stack(st), stack(ns), stack(rw), stack(dn).astype(bool)


def make_model(case):
    """A second env in the same start state whose `replay(actions)` says what the collector's env must have produced."""
    if case["kind"] in ("control", "cartpole"):
        from oracle.jorldy_oracle import CartPoleOracle, ControlOracle

        seed = case_seed(case) % 97
        return _OracleReplay(ControlOracle(case["W"], case["S"], case["A"], seed=seed) if case["kind"] == "control" else CartPoleOracle(case["W"], seed=seed))
    return make_env(case)


# ---------------------------------------------------------------------------------------------- the policies
def network_name(case):
    return "continuous_policy_value" if case["cont"] else "discrete_policy_value"


SHARP_SCALE = 1000.0


def _module(case, pi_scale):
    import fp64_truth as F
    from mirror.networks import Network

    torch.manual_seed(case_seed(case))
    m = Network(network_name(case), case["S"], case["A"], D_hidden=case["H"]).double()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))  # every bias off zero
        if pi_scale != 1.0:
            m.pi.weight.mul_(pi_scale)
            m.pi.bias.mul_(pi_scale)
    F.round_to_fp32_(m)
    return m, F.as32(m)


def policy(case):
    """-> (float64 module with float32-representable weights, its float32 twin)."""
    return _module(case, 1.0)


def sharp(case):
    """The same policy with the `pi` head scaled up: softmax of its logits is a point mass, in float64, on almost every row."""
    assert not case["cont"]
    return _module(case, SHARP_SCALE)


def modules_of(case, state_dict):
    """The float64 / float32 modules that hold `state_dict` (an agent's CURRENT weights)."""
    from mirror.networks import Network

    m64 = Network(network_name(case), case["S"], case["A"], D_hidden=case["H"]).double()
    m64.load_state_dict({k: v.detach().cpu().double() for k, v in state_dict.items()})
    m32 = Network(network_name(case), case["S"], case["A"], D_hidden=case["H"]).float()
    m32.load_state_dict({k: v.detach().cpu().float() for k, v in state_dict.items()})
    return m64, m32


def truths(case, m64, m32, state, next_state):
    """state, next_state [W, T, S] float32 as stored -> {quantity: (float64, torch-cpu-float32)} of h0 [W T, A], h1 (continuous), value [W T] and
    next_value [W T] = V(state[w, t + 1]) for t < T - 1, V(next_state[w, T - 1]) for the last step -- the states the collector queries."""
    W, T, S = state.shape
    x = torch.from_numpy(np.ascontiguousarray(state)).reshape(W * T, S)
    nx = torch.from_numpy(np.concatenate([state[:, 1:], next_state[:, -1:]], axis=1)).reshape(W * T, S)
    out = {}
    with torch.no_grad():
        r64, r32 = m64.raw(x.double()), m32.raw(x)
        out["h0"] = (r64[0], r32[0])
        if case["cont"]:
            out["h1"] = (r64[1], r32[1])
        out["value"] = (r64[-1].reshape(-1), r32[-1].reshape(-1))
        out["next_value"] = (m64.raw(nx.double())[-1].reshape(-1), m32.raw(nx)[-1].reshape(-1))
    return out


def p_max(logits64):
    """[rows, A] float64 logits -> (largest softmax probability, its index) per row."""
    p = torch.softmax(logits64.double(), dim=-1)
    m, i = p.max(dim=-1)
    return m.numpy(), i.numpy()


def greedy_rollout(case, m64, runs=N_RUNS, T=T_STEPS):
    """ScriptedVec rolled with the float64 argmax policy for `runs` runs of T steps -> (states [runs, W, T, S], p_max [runs, W, T])."""
    env = make_env(case)
    W, S = case["W"], case["S"]
    states, pm = np.empty((runs, W, T, S), np.float32), np.empty((runs, W, T))
    nxt, rew, done = np.empty((W, S), np.float32), np.empty(W, np.float32), np.empty(W, np.uint8)
    for r in range(runs):
        for t in range(T):
            x = env.obs()
            with torch.no_grad():
                p, a = p_max(m64.raw(torch.from_numpy(x).double())[0])
            states[r, :, t], pm[r, :, t] = x, p
            env.step(a.astype(np.int64), nxt, rew, done)
    return states, pm
