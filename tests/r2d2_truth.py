"""Float64 statement of R2D2 (core/network/r2d2.py, core/agent/r2d2.py): the comparator of tests/test_r2d2_cpu.py and tests/test_r2d2_gpu.py
(test infrastructure, not the product).

  lstm_cell       one step of torch.nn.LSTM written out: gates = xproj + h W_hh^T, i, f, o = sigmoid, g = tanh, c' = f c + i g, h' = o tanh(c')
  Net             the product's parameter container with a forward: head -> cat[x, prev_action_onehot] -> the explicit recurrence under
                  autograd -> relu(l) -> dueling streams (r2d2.py:28-53); any dtype
  val_rescale / inv_val_rescale   r2d2.py:304-313 AS WRITTEN (in float64 their cancellation costs 1e-13)
  loss            jh_r2d2_loss's contract in numpy float64, from the three time-major Q tensors on
  learn           the whole of R2D2.learn() (r2d2.py:99-163) up to the raw gradients, in the dtype of the networks
and the tables of the kernel tests: STEP_SHAPES, NET_SHAPES, SWEEP with its case builder; beside them the tables at the kernels' own dispatch
limits (EDGE_STEP_SHAPES, EDGE_NET_SHAPE, EDGE_LOSS_CASES) with their builders and the targeted variants of one multi-wave loss case; the reader of the fixtures of
tools/gen_golden_r2d2.py (Fixture) with the generator's fill loop for any agent (fill_loop)."""
import itertools
import os

import numpy as np
import torch
import torch.nn.functional as F

from jorldy_amd.core import network as P

# (rows, H, A): one row and the smallest H; rows and H that are no multiple of the 16 x 16 tile; H = 512 (32 unit tiles, every wave of a
# workgroup takes eight k chunks); more than eight row tiles
STEP_SHAPES = ((1, 4, 2), (5, 36, 5), (3, 512, 2), (130, 64, 3))
# (seq_len, n_burn_in, n_step, B, H, S, A): one trained step; the first fixture's shape; odd everything; the default length
NET_SHAPES = ((2, 1, 1, 1, 4, 3, 2), (4, 1, 3, 8, 64, 4, 3), (6, 3, 2, 7, 36, 5, 5), (80, 40, 4, 2, 64, 4, 2))
# (B, T', A) x (n_step, |Q| scale, eta)
SWEEP_SHAPES = tuple(itertools.product((1, 7, 64), (1, 3, 40), (2, 5)))
SWEEP_VARIANTS = tuple(itertools.product((1, 3), (0.05, 50.0), (0.0, 0.9, 1.0)))
SWEEP_BURN = 2
GAMMA, ALPHA, EPS = 0.997, 0.6, 1e-3


def lstm_cell(xproj, h, c, w_hh):
    """-> (h', c', activated gates [R, 4H] in the order i, f, g, o).  torch tensors of one dtype."""
    H = h.shape[-1]
    pre = xproj + h @ w_hh.t()
    i, f, g, o = torch.sigmoid(pre[..., :H]), torch.sigmoid(pre[..., H:2 * H]), torch.tanh(pre[..., 2 * H:3 * H]), torch.sigmoid(pre[..., 3 * H:])
    c1 = f * c + i * g
    return o * torch.tanh(c1), c1, torch.cat([i, f, g, o], -1)


class Net(P.R2D2):
    def recur(self, x, h, c):
        """x [B, T, H + A], h / c [B, H] -> (outputs [B, T, H], (h, c))."""
        xp = x @ self.lstm.weight_ih_l0.t() + self.lstm.bias_ih_l0 + self.lstm.bias_hh_l0
        out = []
        for t in range(x.shape[1]):
            h, c, _ = lstm_cell(xp[:, t], h, c, self.lstm.weight_hh_l0)
            out.append(h)
        return torch.stack(out, 1), (h, c)

    def forward(self, x1, x2, hidden_in=None):
        """x1 [B, T, S], x2 [B, T, A], hidden_in = (h, c) each [B, H] -> (q [B, T, A], hidden_out)."""
        x = torch.cat([F.relu(self.head.l(x1)), x2], -1)
        if hidden_in is None:
            z = torch.zeros(x.shape[0], self.D_hidden, dtype=x.dtype)
            hidden_in = (z, z)
        x, hidden_out = self.recur(x, *hidden_in)
        x = F.relu(self.l(x))
        x_a = self.l2_a(F.relu(self.l1_a(x)))
        x_a = x_a - x_a.mean(dim=2, keepdim=True)
        return x_a + self.l2_v(F.relu(self.l1_v(x))), hidden_out


def val_rescale(val, eps=1e-3):
    return (val / (abs(val) + 1e-10)) * ((abs(val) + 1) ** (1 / 2) - 1) + (eps * val)


def inv_val_rescale(val, eps=1e-3):
    return (val / (abs(val) + 1e-10)) * ((((1 + 4 * eps * (abs(val) + 1 + eps)) ** (1 / 2) - 1) / (2 * eps)) ** 2 - 1)


def fold(target_q, reward, done, n_burn_in, n_step, seq_len, gamma, eps=1e-3):
    """r2d2.py:131-141 on [B, T', 1] (numpy or torch)."""
    target_q = inv_val_rescale(target_q, eps)
    for i in reversed(range(n_step)):
        target_q = reward[:, i + n_burn_in:i + seq_len] + (1 - done[:, i + n_burn_in:i + seq_len]) * gamma * target_q
    return val_rescale(target_q, eps)


def loss(q, next_q, next_target_q, action, reward, done, weights, n_burn_in, n_step, gamma, eta, alpha, eps=1e-3):
    """q / next_q / next_target_q float32 [T', B, A] time-major; action / reward / done [B, seq_len + n_step - 1]; weights [B]; the scalars
    as float32 values.  -> dict of float64: q_taken, gap (of the two best next actions), target_q, td [B, T'], priority [B], loss, max_Q,
    grad_q [T', B, A]."""
    q, nq, ntq = (np.asarray(v, dtype=np.float32).astype(np.float64).transpose(1, 0, 2) for v in (q, next_q, next_target_q))  # [B, T', A]
    B, T, A = q.shape
    seq_len = T + n_burn_in
    action, reward, done = (np.asarray(v, dtype=np.float32).astype(np.float64).reshape(B, -1, 1) for v in (action, reward, done))
    assert action.shape[1] == seq_len + n_step - 1
    w = np.asarray(weights, dtype=np.float32).astype(np.float64).reshape(B)
    gamma, eta, alpha, eps = (float(np.float32(v)) for v in (gamma, eta, alpha, eps))
    a = np.clip(action[:, n_burn_in:seq_len, 0].astype(np.int64), 0, A - 1)
    bi, ti = np.arange(B)[:, None], np.arange(T)[None, :]
    q_taken = q[bi, ti, a]
    best = nq.argmax(-1)  # the first maximum
    srt = np.sort(nq, -1)
    target_q = fold(ntq[bi, ti, best][..., None], reward, done, n_burn_in, n_step, seq_len, gamma, eps)[..., 0]
    d = q_taken - target_q
    td = np.abs(d)
    prio = (eta * td.max(1) + (1.0 - eta) * td.mean(1)) ** alpha
    g = np.zeros((B, T, A))
    g[np.arange(B), T - 1, a[:, -1]] = 2.0 * w * d[:, -1] / B
    return dict(q_taken=q_taken, gap=srt[..., -1] - srt[..., -2], target_q=target_q, td=td, priority=prio, loss=float((w * td[:, -1] ** 2).mean()),
                max_Q=float(q_taken.max()), grad_q=g.transpose(1, 0, 2))


def sweep_case(B, T, A, n_step, scale, seed=0):
    """Inputs of one jh_r2d2_loss call at SWEEP_BURN burn-in steps: Q values of size `scale`; an episode end inside row 0's trained window;
    where B > 1 the last row left-padded with zeros into its trained window (action, reward, done: what zero_padding stores,
    r2d2.py:207-232)."""
    rs = np.random.RandomState(7919 * seed + 131 * B + 17 * T + 5 * A + n_step + (1 if scale > 1 else 0))
    burn, cols = SWEEP_BURN, SWEEP_BURN + T + n_step - 1
    f = lambda *s: (scale * rs.randn(*s)).astype(np.float32)
    c = dict(B=B, T=T, A=A, n_step=n_step, burn=burn, q=f(T, B, A), next_q=f(T, B, A), next_target_q=f(T, B, A))
    c["action"] = rs.randint(0, A, size=(B, cols)).astype(np.float32)
    c["reward"] = rs.choice([-1.0, 0.0, 1.0, 0.5], size=(B, cols)).astype(np.float32)
    done = (rs.rand(B, cols) < 0.1).astype(np.float32)
    done[0, burn + (T - 1) // 2] = 1.0
    pad = min(cols, burn + (T + 1) // 2) if B > 1 else 0  # (a single row keeps its episode end instead)
    for v in (c["action"], c["reward"], done):
        v[B - 1, :pad] = 0.0
    c["done"] = done
    c["pad"] = pad
    c["weights"] = rs.uniform(0.2, 1.0, size=B).astype(np.float32)
    return c


def sweep_truth(c, eta):
    return loss(c["q"], c["next_q"], c["next_target_q"], c["action"], c["reward"], c["done"], c["weights"], c["burn"], c["n_step"], GAMMA, eta, ALPHA, EPS)


# ---------------------------------------------------------------------------------------------- the kernels' own dispatch edges
# (rows, H, A) of tests/test_r2d2_edges_gpu.py.  jh_lstm_step splits ceil(H / 16) k chunks over four waves and owns 16 rows x 16 units per
# workgroup: H 8 half a unit tile; 16 one tile, one chunk; 20 two chunks, the second with 4 live k, the second unit tile with 4 units; 48 three
# chunks (wave 3 idle); 52 four, the last partial; 68 five (wave 0 takes two, the others one); 100 seven (three waves take two); 1024 sixteen
# per wave.  Every H meets one of the rows 15 / 16 / 17, rows 1 and 33 (three row tiles) a few of them.
EDGE_STEP_SHAPES = ((15, 8, 2), (16, 16, 3), (1, 16, 2), (17, 20, 5), (1, 20, 2), (15, 48, 2), (16, 52, 3), (17, 68, 2), (33, 68, 3), (15, 100, 4), (1, 100, 2),
                    (17, 1024, 2))
# the network object beside NET_SHAPES (seq_len, n_burn_in, n_step, B, H, S, A): two row tiles with one row in the second, a partial unit tile
# and a partial k chunk at every one of its three-segment step launches
EDGE_NET_SHAPE = (5, 2, 2, 17, 20, 3, 4)
# (B, T', A, n_step, seed) at SWEEP_BURN burn-in steps, both |Q| scales, eta 0.9: every wave count edge of the one-workgroup loss kernel
# (B <= 1024 = 16 waves), the widest A, T' + burn-in = 128, n_step > T' and n_step at its cap.  The seed is the first one at which
# test_r2d2_cpu's two conditions on these cases hold: off every discontinuity, and a loss that a lost wave would miss by ten times the
# tolerance (both decided by the float64 truth alone).
EDGE_LOSS_CASES = ((65, 1, 2, 1, 1), (128, 3, 5, 3, 0), (255, 3, 64, 5, 0), (256, 1, 18, 5, 0), (257, 3, 2, 3, 0), (1023, 1, 5, 1, 0), (1024, 1, 64, 3, 0),
                   (1024, 3, 18, 1, 1), (64, 40, 64, 3, 0), (256, 40, 5, 3, 1), (2, 126, 5, 3, 0), (65, 126, 2, 1, 0), (7, 1, 2, 128, 0))
EDGE_SCALES = (0.05, 50.0)
EDGE_ETA = 0.9
EDGE_MULTI = (1024, 3, 18, 1, 1)  # the multi-wave case of the targeted variants; it also runs at eta 0 and 1


def step_case(rows, H, A, seed):
    """One row group of a jh_lstm_step launch in float64, rounded to float32 values (test_r2d2_gpu._step_case's construction): xproj = x W_ih^T +
    b_ih + b_hh from an input row of H + A entries, W_hh in torch.nn.LSTM's initial range."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + H + A)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    k = 1.0 / np.sqrt(H)
    w_ih, w_hh, b = k * r(4 * H, H + A), k * r(4 * H, H), k * r(4 * H)
    xproj = (r(rows, H + A) @ w_ih.t() + b).float().double()
    return dict(xproj=xproj, w_hh=w_hh.float().double(), h=(0.5 * r(rows, H)).float().double(), c=r(rows, H).float().double())


def edge_step_groups(rows, H, A):
    """The four row groups of one launch, each with weights of its own: rows, none (the empty segment in the middle), rows + 3, one."""
    return [step_case(n, H, A, 11 + s) for s, n in enumerate((rows, 0, rows + 3, 1))]


def _copy(c):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}


def taken(c):
    """[B, T'] the action of every trained step as the kernel reads it (clamped into [0, A))."""
    return np.clip(c["action"][:, c["burn"]:c["burn"] + c["T"]].astype(np.int64), 0, c["A"] - 1)


def with_max_q_at(c, row, t=0):
    """The taken-action q of (row, step t) raised above every other entry -> (case, that float32 value): max_Q must be exactly it."""
    c = _copy(c)
    v = np.float32(4.0 * np.abs(c["q"]).max())
    c["q"][t, row, taken(c)[row, t]] = v
    return c, v


def with_one_weight(c, wave):
    """Every importance weight zero but one of wave `wave` (rows 64 wave ..): the row of that wave whose last-step |td| is largest in the float64
    truth, at weight 1 -> (case, row).  The loss is then one term that only the cross-wave sum can deliver to thread 0."""
    c = _copy(c)
    t = sweep_truth(c, EDGE_ETA)
    lo, hi = 64 * wave, min(c["B"], 64 * wave + 64)
    row = lo + int(np.argmax(t["td"][lo:hi, -1]))
    c["weights"][:] = 0.0
    c["weights"][row] = 1.0
    return c, row


def variant_rows(B):
    """Six rows away from row 0 (the episode end) and row B - 1 (the padded one); beyond one wave three of them sit in the last wave."""
    return (1, 2, 3, B - 4, B - 3, B - 2) if B > 64 else (1, 2, 3, 4, 5, 6)


def with_bad_actions(c):
    """Stored actions out of range over the whole trained window of six rows: -1, A, A + 3, -1, A, A + 3 -> (case, {row: the column the
    kernel's documented clamp lands on}).  r2d2_truth.loss clips the same way."""
    c = _copy(c)
    want = {}
    for i, row in enumerate(variant_rows(c["B"])):
        v = (-1.0, float(c["A"]), float(c["A"] + 3))[i % 3]
        c["action"][row, c["burn"]:c["burn"] + c["T"]] = v
        want[row] = 0 if v < 0 else c["A"] - 1
    return c, want


def with_exact_ties(c):
    """In six rows, at every trained step, the second-best next_q entry set to the best one's float32 value, and next_target_q at those two
    actions set to + and - max |next_target_q| (the lower index gets the +): `first maximum` decides the target by twice that -> (case, rows)."""
    c = _copy(c)
    rows = variant_rows(c["B"])
    scale = np.float32(np.abs(c["next_target_q"]).max())
    for row in rows:
        for t in range(c["T"]):
            k2, k1 = np.argsort(c["next_q"][t, row], kind="stable")[-2:]
            c["next_q"][t, row, k2] = c["next_q"][t, row, k1]
            lo, hi = min(k1, k2), max(k1, k2)
            c["next_target_q"][t, row, lo], c["next_target_q"][t, row, hi] = scale, -scale
    return c, rows


def with_all_done(c, row):
    """done = 1 at every column of `row`: its targets are the rescaled rewards alone."""
    c = _copy(c)
    c["done"][row, :] = 1.0
    return c


def edge_multi_variants(scale):
    """The targeted variants of EDGE_MULTI at one |Q| scale -> [(name, case, what the variant pins down)]: the global max_Q in the last wave's
    last row, in the first row of a middle wave and in row 0; all of the loss in one row of the last and of a middle wave; actions out of
    range; exact next_q ties; a row that is done at every column."""
    B, T, A, n_step, seed = EDGE_MULTI
    c = sweep_case(B, T, A, n_step, scale, seed)
    out = []
    for row in (B - 1, 64 * 7, 0):
        cc, v = with_max_q_at(c, row)
        out.append((f"max_Q in row {row}", cc, dict(max_q=v, row=row)))
    for wave in (15, 9):
        cc, row = with_one_weight(c, wave)
        out.append((f"the only weight in wave {wave}", cc, dict(only_row=row)))
    cc, want = with_bad_actions(c)
    out.append(("actions out of range", cc, dict(columns=want)))
    cc, rows = with_exact_ties(c)
    out.append(("exact ties", cc, dict(tie_rows=rows)))
    out.append(("a row done at every column", with_all_done(c, 5), dict(done_row=5)))
    return out


def batch(rs, B, seq_len, n_step, S, A, H, pad_rows=(), done_rows=()):
    """One sampled batch as R2D2.learn() receives it after stacking (float32 numpy): state [B, L, S], prev_action_onehot [B, L, A], action /
    reward / done [B, L - 1, 1], the four stored hidden states [B, 1, H], L = seq_len + n_step.  pad_rows are left-padded with zeros over
    their first half, done_rows end an episode in the middle of the window."""
    L = seq_len + n_step
    act = rs.randint(0, A, size=(B, L))
    b = {"state": rs.randn(B, L, S).astype(np.float32), "action": act[:, 1:, None].astype(np.float32),
         "prev_action_onehot": np.eye(A, dtype=np.float32)[act], "reward": rs.choice([-1.0, 0.0, 1.0, 0.5], size=(B, L - 1, 1)).astype(np.float32),
         "done": np.zeros((B, L - 1, 1), np.float32)}
    for k in ("hidden_h", "hidden_c", "next_hidden_h", "next_hidden_c"):
        b[k] = (0.3 * rs.randn(B, 1, H)).astype(np.float32)
    for r in done_rows:
        b["done"][r, (L - 1) // 2] = 1.0
    for r in pad_rows:
        n = L // 2
        for k in ("state", "prev_action_onehot"):
            b[k][r, :n] = 0.0
        for k in ("action", "reward", "done"):
            b[k][r, :n] = 0.0
    return b


def passes(net, target, b, seq_len, n_burn_in, n_step):
    """The three sequence passes of learn() (r2d2.py:117-129) in the dtype of `net`, each through get_q (r2d2.py:289-302: the burn-in steps
    run without gradient and only hand over the state) -> (q_pred with its graph, next_q, next_target_q), each [B, T', A]; t = the batch as
    tensors."""
    dt = next(net.parameters()).dtype
    t = {k: torch.as_tensor(np.asarray(v)).to(dt) for k, v in b.items()}
    hid = lambda k: (t[k + "_h"][:, 0], t[k + "_c"][:, 0])

    def get_q(state, pa, hidden, network):
        with torch.no_grad():
            _, hidden = network(state[:, :n_burn_in], pa[:, :n_burn_in], hidden)
        return network(state[:, n_burn_in:], pa[:, n_burn_in:], hidden)[0]

    state, pa = t["state"][:, :seq_len], t["prev_action_onehot"][:, :seq_len]
    nstate, npa = t["state"][:, n_step:], t["prev_action_onehot"][:, n_step:]
    q_pred = get_q(state, pa, hid("hidden"), net)
    with torch.no_grad():
        next_q = get_q(nstate, npa, hid("next_hidden"), net)
        next_target_q = get_q(nstate, npa, hid("next_hidden"), target)
    return q_pred, next_q, next_target_q, t


def learn(net, target, b, weights, seq_len, n_burn_in, n_step, gamma, eta, alpha, eps=1e-3):
    """R2D2.learn() (r2d2.py:99-159) on the batch `b` (batch()'s layout) in the dtype of `net`; leaves the raw gradients in net's .grad.
    -> dict of detached tensors: q [B, T', 1], next_q, next_target_q [B, T', A], target_q, td_error [B, T', 1], priority [B, 1], loss, max_Q."""
    for p in net.parameters():
        p.grad = None
    q_pred, next_q, next_target_q, t = passes(net, target, b, seq_len, n_burn_in, n_step)
    dt, A = q_pred.dtype, q_pred.shape[-1]
    eye = torch.eye(A, dtype=dt)
    one_hot = eye[t["action"][:, :seq_len].reshape(-1, seq_len).long()][:, n_burn_in:]
    q = (q_pred * one_hot).sum(-1, keepdims=True)
    with torch.no_grad():
        target_q = (next_target_q * eye[torch.argmax(next_q, -1)]).sum(-1, keepdims=True)
        target_q = fold(target_q, t["reward"], t["done"], n_burn_in, n_step, seq_len, gamma, eps)
    td = abs(target_q - q)
    prio = torch.pow(eta * torch.max(td, axis=1).values + (1 - eta) * torch.mean(td, axis=1), alpha)
    w = torch.as_tensor(np.asarray(weights)).to(dt).reshape(-1, 1)
    ls = (w * (td[:, -1] ** 2)).mean()
    ls.backward()
    d = lambda v: v.detach()
    return dict(q=d(q), q_pred=d(q_pred), next_q=d(next_q), next_target_q=d(next_target_q), target_q=d(target_q), td_error=d(td), priority=d(prio), loss=float(ls.detach()),
                max_Q=float(q.detach().max()))


# ---------------------------------------------------------------------------------------------- the fixtures of tools/gen_golden_r2d2.py
FIXTURES = ("r2d2", "r2d2_odd", "r2d2_cartpole")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCALED = ("l2_a.weight", "l2_a.bias", "l2_v.weight", "l2_v.bias")
ROW_KEYS = ("hidden_h", "hidden_c", "next_hidden_h", "next_hidden_c", "state", "reward", "done", "action", "prev_action_onehot")


class Fixture:
    def __init__(self, name):
        self.name, self.z = name, np.load(os.path.join(GOLDEN, name + ".npz"))
        h = lambda k: self.z[f"hyper/{k}"]
        for k in ("S", "A", "H", "B", "seq_len", "n_burn_in", "n_step", "steps", "episode", "trace", "thin_stride", "thin_limit", "act_np_seed", "fill_seed",
                  "recipe_seed", "init_seed", "np_seed", "n_rows", "zero_padding"):
            setattr(self, k, int(h(k)))
        for k in ("lr", "beta", "alpha", "eta", "gamma", "clip_grad_norm", "epsilon", "q_scale", "ref_target_err"):
            setattr(self, k, float(h(k)))
        # the target-dependent quantities of the cartpole fixture: the reference's own float32 distance from float64 decides (the issue's bound)
        self.target_tol = 2.0 * self.ref_target_err + 1e-5 if name == "r2d2_cartpole" else 1e-5

    def thin(self, a):
        from oracle import synth

        return synth.thin(np.asarray(a), self.thin_limit, self.thin_stride)

    def agent_kwargs(self, **over):
        kw = dict(state_size=self.S, action_size=self.A, hidden_size=self.H, network="r2d2", head="mlp", optim_config={"name": "adam", "lr": self.lr}, gamma=self.gamma,
                  buffer_size=256, batch_size=self.B, clip_grad_norm=self.clip_grad_norm, start_train_step=0, target_update_period=10000, lr_decay=False,
                  n_step=self.n_step, alpha=self.alpha, beta=self.beta, uniform_sample_prob=1e-3, seq_len=self.seq_len, n_burn_in=self.n_burn_in,
                  zero_padding=bool(self.zero_padding), epsilon=self.epsilon, eta=self.eta, run_step=100000)
        kw.update(over)
        return kw

    def weights(self, which):
        """The starting weights of the online (0) / target (1) network: the recipe's, the streams' last layers scaled by hyper/q_scale."""
        from oracle import synth

        shapes = {k[len("shape/"):]: tuple(int(x) for x in self.z[k]) for k in self.z.files if k.startswith("shape/")}
        sd = synth.recipe_state_dict(shapes, self.recipe_seed + which)
        for k in SCALED:
            sd[k] = np.ascontiguousarray(sd[k] * np.float32(self.q_scale), dtype=np.float32)
        return {k: torch.from_numpy(v) for k, v in sd.items()}

    def learn(self, k):
        p = f"l{k}/"
        return {key[len(p):]: self.z[key] for key in self.z.files if key.startswith(p)}

    def rows(self):
        """The stored rows in full (the two small fixtures keep every column whole) -> {key: [n_rows, ...]} or None where they are thinned."""
        L = self.seq_len + self.n_step
        shp = {"state": (L, self.S), "prev_action_onehot": (L, self.A), "action": (L - 1, 1), "reward": (L - 1, 1), "done": (L - 1, 1)}
        out = {}
        for k in ROW_KEYS:
            a = self.z["rows/" + k]
            want = (self.n_rows,) + shp.get(k, (1, self.H))
            if a.size != int(np.prod(want)):
                return None
            out[k] = a.reshape(want)
        return out


def fill_loop(agent, f, store=True):
    """tools/gen_golden_r2d2.py's fill loop for any agent with the reference's interface -> (act()'s outputs per step, the emitted rows)."""
    rs = np.random.RandomState(f.fill_seed)
    np.random.seed(f.act_np_seed)
    state, trace, rows = rs.randn(1, f.S).astype(np.float32), [], []
    for t in range(f.steps):
        out = agent.act(state, True)
        nxt = rs.randn(1, f.S).astype(np.float32)
        done = (t + 1) % f.episode == 0
        tr = {"state": state, "next_state": nxt, "reward": np.asarray([[rs.choice([-1.0, 0.0, 1.0, 0.5])]], np.float32), "done": np.asarray([[done]])}
        tr.update(out)
        trace.append(dict(out, state=state, done=np.asarray(done)))
        row = agent.interact_callback(tr)
        if row:
            rows.append(row)
            if store:
                agent.memory.store([row])
        state = nxt
    return trace, rows
