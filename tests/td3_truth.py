"""Float64 restatement of deterministic actor-critic learning (core/agent/td3.py:146-209, core/agent/ddpg.py:117-163) with torch autograd on
the CPU: the comparator of tests/test_td3_cpu.py and tests/test_td3_gpu.py (test infrastructure, not the product).  Every function takes
`dtype`: torch.float64 is the truth, torch.float32 the torch-CPU-fp32 comparator that fp64_truth.vs_exact's criterion needs.

  Actor / Critic        forward-capable mirrors of network/policy.py:8-20 and network/q_network.py:23-39 under the reference's keys
  next_action           clamp(tanh(z) + clamp(std * eps, -c, c), -1, 1); eps None: tanh(z)
  critic_loss           y, the n losses, max_Q and d(loss_i)/d(q_i) from q, q_next [n, B]
  actor_seed            actor_loss = -mean(q) and its gradient
  critic_update         one whole critic update given state dicts, a batch and the noise: y, q_i, losses, max_Q, parameter gradients
  actor_update          one whole actor update: actor(s), actor_loss, the actor's parameter gradients (through critic 1's action input)
  adam_first_step       a fresh Adam's first step: critic 1 as the actor update sees it
  polyak                the reference's expression tau * p + (1 - tau) * t on tensors of the given dtype
and the sweep generators of the kernel tests."""
from collections import OrderedDict

import numpy as np
import torch


class _Head(torch.nn.Module):
    def __init__(self, S, H):
        super().__init__()
        self.l = torch.nn.Linear(S, H)


class Actor(torch.nn.Module):
    def __init__(self, S, A, H):
        super().__init__()
        self.head = _Head(S, H)
        self.l = torch.nn.Linear(H, H)
        self.pi = torch.nn.Linear(H, A)

    def pre(self, x):
        return self.pi(torch.relu(self.l(torch.relu(self.head.l(x)))))

    def forward(self, x):
        return torch.tanh(self.pre(x))


class Critic(torch.nn.Module):
    def __init__(self, S, A, H):
        super().__init__()
        self.head = _Head(S, H)
        self.e = torch.nn.Linear(A, H)
        self.l = torch.nn.Linear(2 * H, H)
        self.q = torch.nn.Linear(H, 1)

    def forward(self, x, a):
        cat = torch.cat([torch.relu(self.head.l(x)), torch.relu(self.e(a))], dim=-1)
        return self.q(torch.relu(self.l(cat)))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)).to(dtype)


def build(cls, sd, dtype):
    """A mirror module of `cls` holding the state dict `sd` (arrays or tensors, the reference's keys) in `dtype`."""
    S = int(np.shape(sd["head.l.weight"])[1])
    H = int(np.shape(sd["head.l.weight"])[0])
    A = int(np.shape(sd["pi.weight"])[0]) if cls is Actor else int(np.shape(sd["e.weight"])[1])
    m = cls(S, A, H).to(dtype)
    m.load_state_dict(OrderedDict((k, _t(v, dtype)) for k, v in sd.items()))
    return m


def next_action(z, eps, std, clip, dtype=torch.float64):
    a = torch.tanh(_t(z, dtype))
    if eps is None:
        return a
    noise = (_t(eps, dtype) * std).clamp(-clip, clip)
    return (a + noise).clamp(-1.0, 1.0)


def critic_loss(q, q_next, reward, done, gamma, dtype=torch.float64):
    """q, q_next [n, B] -> dict(y [B], loss [n], max_Q, grad [n, B])."""
    q = _t(q, dtype).clone().requires_grad_(True)
    qn, r, d = _t(q_next, dtype), _t(reward, dtype).reshape(-1), _t(done, dtype).reshape(-1)
    y = r + (1 - d) * gamma * qn.min(dim=0).values
    losses = [torch.nn.functional.mse_loss(y, q[i]) for i in range(q.shape[0])]
    sum(losses).backward()
    return dict(y=y.detach(), loss=torch.stack(losses).detach(), max_Q=y.max().detach(), grad=q.grad.detach())


def actor_seed(q, dtype=torch.float64):
    q = _t(q, dtype).reshape(-1).clone().requires_grad_(True)
    loss = -q.mean()
    loss.backward()
    return dict(actor_loss=loss.detach(), grad=q.grad.detach())


def critic_update(sd_target_actor, sd_critics, sd_target_critics, state, action, reward, next_state, done, noise, gamma, noise_std, noise_clip, dtype=torch.float64):
    """td3.py:157-176 (two critics) / ddpg.py:128-138 (one critic, noise None).  sd_critics / sd_target_critics: lists of state dicts.
    -> dict(next_action, y, q [n][B, 1], loss [n], max_Q, grads [n]{name: tensor})."""
    ta = build(Actor, sd_target_actor, dtype)
    cs = [build(Critic, sd, dtype) for sd in sd_critics]
    tcs = [build(Critic, sd, dtype) for sd in sd_target_critics]
    s, a, r, s2, d = _t(state, dtype), _t(action, dtype), _t(reward, dtype).reshape(-1, 1), _t(next_state, dtype), _t(done, dtype).reshape(-1, 1)
    with torch.no_grad():
        a2 = next_action(ta.pre(s2), noise, noise_std, noise_clip, dtype)
        nq = torch.stack([tc(s2, a2) for tc in tcs]).min(dim=0).values
        y = r + (1 - d) * gamma * nq
    qs, losses, grads = [], [], []
    for c in cs:
        q = c(s, a)
        loss = torch.nn.functional.mse_loss(y, q)
        loss.backward()
        qs.append(q.detach())
        losses.append(loss.detach())
        grads.append(OrderedDict((k, p.grad.detach().clone()) for k, p in c.named_parameters()))
    return dict(next_action=a2, y=y, q=qs, loss=losses, max_Q=y.max(), grads=grads)


def actor_update(sd_actor, sd_critic1, state, dtype=torch.float64):
    """td3.py:181-188 / ddpg.py:143-148.  -> dict(action_pred, actor_loss, grads {name: tensor}: the ACTOR's parameter gradients)."""
    actor, c1 = build(Actor, sd_actor, dtype), build(Critic, sd_critic1, dtype)
    s = _t(state, dtype)
    a = actor(s)
    loss = -c1(s, a).mean()
    loss.backward()
    return dict(action_pred=a.detach(), actor_loss=loss.detach(), grads=OrderedDict((k, p.grad.detach().clone()) for k, p in actor.named_parameters()))


def adam_first_step(sd, grads, lr, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64):
    """The first step of a fresh torch.optim.Adam on the parameters `sd` with the gradients `grads` (both {name: array}), in `dtype`:
    what critic_optimizer1.step() leaves behind (td3.py:178 / ddpg.py:140) in front of the actor update.  -> the stepped state dict."""
    params = OrderedDict((k, torch.nn.Parameter(_t(v, dtype).clone())) for k, v in sd.items())
    for k, p in params.items():
        p.grad = _t(grads[k], dtype).clone().reshape(p.shape)
    torch.optim.Adam(list(params.values()), lr=lr, betas=betas, eps=eps).step()
    return OrderedDict((k, p.detach().clone()) for k, p in params.items())


def polyak(p, t, tau):
    """The reference's expression (td3.py:205), evaluated by torch on tensors of the dtype given."""
    return tau * p + (1 - tau) * t


# ---------------------------------------------------------------------------------------------- sweep generators
NEXT_ACTION_SHAPES = ((1, 1), (7, 3), (128, 6), (1025, 17))
CRITIC_LOSS_B = (1, 7, 128, 1025)
CRITIC_LOSS_VARIANTS = ("plain", "all_done", "equal_targets")
STD, CLIP = 0.2, 0.5


def next_action_case(B, A, seed=0):
    """z, eps float32 [B, A] with BOTH clamps of next_action active on BOTH sides: the first two elements are set by hand -- (z, eps) =
    (3, 4): noise above the inner bound and tanh(z) + 0.5 above 1; (-3, -4): the mirror image -- and the rest is random with wide tails.
    A single element can sit on one side only: next_action_cases gives shape (1, 1) one case per side."""
    rng = np.random.RandomState(1000 * B + A + seed)
    z = (rng.randn(B, A) * 1.5).astype(np.float32)
    eps = (rng.randn(B, A) * 2.0).astype(np.float32)
    forced = [(3.0, 4.0), (-3.0, -4.0)]
    zf, ef = z.reshape(-1), eps.reshape(-1)
    for i in range(min(zf.size, 2)):
        zf[i], ef[i] = forced[(i + seed) % 2]
    return z, eps


def next_action_cases(B, A):
    return [next_action_case(B, A, s) for s in ((0, 1) if B * A < 2 else (0,))]


def clamps_active(z, eps, std=STD, clip=CLIP):
    """-> (inner high, inner low, outer high, outer low) counts of one case."""
    n = eps.astype(np.float64) * std
    a = np.tanh(z.astype(np.float64)) + np.clip(n, -clip, clip)
    return int((n > clip).sum()), int((n < -clip).sum()), int((a > 1).sum()), int((a < -1).sum())


def critic_loss_case(B, n, variant, seed=0):
    rng = np.random.RandomState(77 * B + 5 * n + seed)
    q = rng.randn(n, B).astype(np.float32) * 2
    qn = rng.randn(n, B).astype(np.float32) * 2
    if variant == "equal_targets" and n == 2:
        qn[1] = qn[0]
    r = rng.choice([-1.0, 0.0, 1.0, 0.5], size=B).astype(np.float32)
    d = np.ones(B, np.float32) if variant == "all_done" else (rng.rand(B) < 0.2).astype(np.float32)
    return q, qn, r, d


# ---------------------------------------------------------------------------------------------- fixtures (tools/gen_golden_td3.py)
FIXTURES = ("td3", "td3_odd", "td3_cartpole", "ddpg", "ddpg_pendulum")
FIXTURE_NETS = {"td3": ("actor", "target_actor", "critic1", "target_critic1", "critic2", "target_critic2"), "ddpg": ("actor", "target_actor", "critic", "target_critic")}
ACTOR_KEYS = ("head.l.weight", "head.l.bias", "l.weight", "l.bias", "pi.weight", "pi.bias")
CRITIC_KEYS = ("head.l.weight", "head.l.bias", "e.weight", "e.bias", "l.weight", "l.bias", "q.weight", "q.bias")


def shapes_of(net, S, A, H):
    if "actor" in net:
        return OrderedDict(zip(ACTOR_KEYS, ((H, S), (H,), (H, H), (H,), (A, H), (A,))))
    return OrderedDict(zip(CRITIC_KEYS, ((H, S), (H,), (H, A), (H,), (H, 2 * H), (H,), (1, H), (1,))))


class Fixture:
    """One fixture file: the starting weights of every network in full (stored, or regenerated from the recipe and checked against the
    stored sample), the thinning rule of everything else, and the records."""

    def __init__(self, z):
        from oracle import synth

        self.z, self.kind = z, str(z["hyper/agent"])
        self.S, self.A, self.H, self.B = (int(z[f"hyper/{k}"]) for k in ("S", "A", "H", "B"))
        self.limit = int(z["hyper/thin_limit"])
        self.nets = FIXTURE_NETS[self.kind]
        self.records = sorted({k.split("/")[0] for k in z.files if k.startswith("r") and k.split("/")[0][1:].isdigit()})
        self.sd0 = {}
        for i, net in enumerate(self.nets):
            shapes = shapes_of(net, self.S, self.A, self.H)
            if int(z["hyper/recipe"]):
                sd = synth.recipe_state_dict(shapes, int(z["hyper/recipe_seed"]) + i)
                for k, v in sd.items():
                    assert np.array_equal(self.thin(v), z[f"sd0/{net}/{k}"]), (net, k)
            else:
                sd = OrderedDict((k, z[f"sd0/{net}/{k}"]) for k in shapes)
                assert all(tuple(sd[k].shape) == tuple(s) for k, s in shapes.items())
            self.sd0[net] = OrderedDict((k, np.asarray(sd[k], dtype=np.float32)) for k in shapes)

    def thin(self, a):
        from oracle import synth

        a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a)
        return synth.thin(a, self.limit) if self.limit else a

    def critics(self, target=False):
        names = ("critic1", "critic2") if self.kind == "td3" else ("critic",)
        return [("target_" + n) if target else n for n in names]

    def batch(self, r):
        return {k: self.z[f"{r}/learn/{k}"] for k in ("state", "action", "reward", "next_state", "done")}

    def eps(self, r):
        return self.z[f"{r}/learn/eps"] if self.kind == "td3" else None

    def noise_args(self):
        return (float(self.z["hyper/target_noise_std"]), float(self.z["hyper/target_noise_clip"])) if self.kind == "td3" else (0.0, 0.0)

    def has_actor_step(self, r):
        return f"{r}/learn/actor_loss" in self.z.files

    def unchanged(self, r, net):
        return bool(int(self.z[f"{r}/unchanged/{net}"]))

    def buffer(self):
        """The stored transitions as the list of dicts an agent's process / memory.store takes."""
        z = self.z
        n = len(z["buf_state"])
        return [{k: z[f"buf_{k}"][i : i + 1] for k in ("state", "action", "reward", "next_state", "done")} for i in range(n)]
