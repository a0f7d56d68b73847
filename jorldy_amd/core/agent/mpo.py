import os
from collections import deque

import numpy as np
import torch

from ... import ops
from ..buffer import ReplayBuffer
from ..buffer.base import h2d_small
from ..network import Network
from ..optimizer import Optimizer
from . import optim_state
from .base import BaseAgent
from .native_net import NativeNet, load_moments, moments_of, shadow_of

MAX_ROWS = 1024  # jh_mpo_loss_discrete: one workgroup, one row of the batch_size x n_step trajectories per thread
MAX_ACTIONS = 64  # logits per row the loss kernel loops over
MPO_ELIGIBLE = ("MPO runs on libjorldy_hip only: actor 'discrete_policy' with critic 'discrete_q_network', head 'mlp' with a scalar state_size, "
                "hidden_size % 4 == 0, optim_config {'name': 'adam', lr, betas, eps}, critic_loss_type in {'retrace', '1step_TD'}, "
                f"2 <= action_size <= {MAX_ACTIONS} and batch_size * n_step <= {MAX_ROWS} (n_step counts as 1 with '1step_TD'): the Retrace scan and every "
                "mean of a learn() run inside one workgroup (config.mpo.cartpole / mountaincar / pong_mlagent and their shapes); 'continuous_policy', "
                "the cnn head and data-parallel learners (grad_sync) are not available for this agent -- except that actor 'continuous_policy' together "
                f"with critic 'continuous_q_network' runs under the same head, hidden_size, optimizer and row rules at 1 <= action_size <= {ops.MPO_MAX_CONT_ACTIONS}, "
                f"num_sample >= 1 and num_sample * batch_size * n_step <= {ops.MPO_MAX_SAMPLED} sampled rows (config.mpo.pendulum: 7680, hopper_mlagent / "
                "drone_delivery_mlagent: 960; the class defaults' 30 * 64 * 8 = 15360 are refused); a continuous actor with a discrete critic, or the reverse, is refused")


class MPO(BaseAgent):
    """core/agent/mpo.py:14-484 for a discrete policy, on the native engine.

      networks      actor (discrete_policy) and critic (discrete_q_network) have one shape: head -> l -> A outputs.  Each lives in an
                    ops.RainbowNet of its own (kind "pi" / "q") with its online and target buckets, backward, clip and Adam.  Constructed in
                    the reference's order (actor, target actor, critic, target critic: mpo.py:93-109), so that one torch.manual_seed gives
                    the same initial weights.
      replay        the reference's ReplayBuffer of whole trajectories: every column is [T, dim] per stored row (interact_callback stacks a
                    sliding window of n_step transitions that is not reset at episode ends, mpo.py:477-484); np.random.randint draws the rows.
      learn()       gather into ONE contiguous [s; s'] batch of 2R rows (R = batch_size * T) -> the actor's three forwards online(s), online(s'),
                    target(s) (jh_rbnet_learn_forward_p) -> the critic's online(s), target(s), target(s') (jh_rbnet_learn_forward_m) ->
                    jh_mpo_loss_discrete (Retrace, the four losses, both head gradients, AND the multipliers' Adam steps and floors on the
                    device) -> two backwards -> two clip_grad_norm_ + Adam, each over its own network's parameters only (mpo.py:386-395).
                    One hipGraph after a warm eager call.
      multipliers   eta, alpha_mu, alpha_sigma live in V-MPO's device block (ops.vmpo_block), stepped by the loss kernel with the ACTOR's lr,
                    betas, eps and step count (the actor's optimizer holds them, mpo.py:142-146; the cosine decay reaches them through the
                    actor's hyper block).  Learn k sees them after k - 1 steps.  alpha_sigma has no gradient for a discrete policy.
      process()     store, then n_epoch learns (each followed by the lr decay) and ONE hard target update of both nets (mpo.py:447-463); the
                    statistics of the last learn are read back once.

    Departures on purpose: log pi is a log-softmax and eta_loss's log-sum is formed around the row maximum (finite where the reference's float32
    overflows or underflows, equal elsewhere); act() returns each row's OWN probability where the reference's np.take(pi, action) reads row 0's
    for every row (identical at one row).  save() / load() are the reference's four keys; the multipliers' VALUES are not part of it (their
    Adam moments are); save_full / load_full carry the whole block."""

    action_type = "discrete"

    def __new__(cls, state_size=None, action_size=None, hidden_size=512, optim_config=None, actor="discrete_policy", *args, **kwargs):
        """Agent("mpo", actor="continuous_policy", ...) is the sibling class below; everything else, refusals included, is this one."""
        return object.__new__(MPOContinuous if cls is MPO and actor == "continuous_policy" else cls)

    def __init__(self, state_size, action_size, hidden_size=512, optim_config={"name": "adam"}, actor="discrete_policy", critic="discrete_q_network",
                 head="mlp", buffer_size=50000, batch_size=64, start_train_step=2000, n_epoch=64, n_step=8, clip_grad_norm=1.0, gamma=0.99, run_step=1e6,
                 lr_decay=True, device=None, critic_loss_type="retrace", num_sample=30, min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.01,
                 eps_alpha_mu=0.01, eps_alpha_sigma=5 * 1e-5, eta=1.0, alpha_mu=1.0, alpha_sigma=1.0, use_graph=True, **kwargs):
        T = n_step if critic_loss_type == "retrace" else 1
        is_int = lambda v: isinstance(v, (int, np.integer))
        ok = (head == "mlp" and np.isscalar(state_size) and is_int(hidden_size) and hidden_size % 4 == 0 and isinstance(optim_config, dict)
              and str(optim_config.get("name", "adam")).lower() == "adam" and set(optim_config) <= {"name", "lr", "betas", "eps"}
              and critic_loss_type in ("retrace", "1step_TD") and is_int(action_size) and is_int(batch_size) and is_int(T) and batch_size >= 1 and T >= 1
              and batch_size * T <= MAX_ROWS and kwargs.get("grad_sync") is None and self._eligible(actor, critic, action_size, num_sample, batch_size * T))
        if not ok:
            raise ValueError(f"{MPO_ELIGIBLE}; got actor={actor!r}, critic={critic!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size!r}, "
                             f"optim_config={optim_config!r}, critic_loss_type={critic_loss_type!r}, action_size={action_size!r}, batch_size={batch_size!r}, "
                             f"n_step={n_step!r}, num_sample={num_sample!r}")
        self.device = self._require_gpu(device)
        self.use_graph = use_graph
        self.grad_sync = None
        self.head, self.action_size, self.state_size, self.hidden_size = head, int(action_size), int(state_size), int(hidden_size)
        self.critic_loss_type = critic_loss_type
        self.batch_size, self.n_step, self.clip_grad_norm, self.num_sample = int(batch_size), int(T), clip_grad_norm, num_sample
        # mpo.py:93-109: four constructions in this order; the targets' own initialisations are drawn and then overwritten
        inits = [Network(name, state_size, action_size, D_hidden=hidden_size, head=head) for name in (actor, actor, critic, critic)]
        self._actor, self._critic = self._build_nets(self.batch_size * self.n_step)
        for net, init in ((self._actor, inits[0]), (self._critic, inits[2])):
            net.import_state(init.state_dict())
            net.sync_target()
        self._net = self._actor  # the marker of a native agent
        self.actor, self.target_actor = NativeNet(self._actor, 0), NativeNet(self._actor, 1)
        self.critic, self.target_critic = NativeNet(self._critic, 0), NativeNet(self._critic, 1)
        self.num_learn, self.time_t = 0, 0
        self.start_train_step, self.n_epoch = start_train_step, int(n_epoch)
        self.min_eta, self.min_alpha_mu, self.min_alpha_sigma = min_eta, min_alpha_mu, min_alpha_sigma
        self.eps_eta, self.eps_alpha_mu, self.eps_alpha_sigma = eps_eta, eps_alpha_mu, eps_alpha_sigma
        self._mult = ops.vmpo_block(eta, alpha_mu, alpha_sigma, min_eta, min_alpha_mu, min_alpha_sigma, eps_eta, eps_alpha_mu, eps_alpha_sigma, device=self.device)
        self._optim_config = dict(optim_config)
        d = Optimizer(**optim_config, params=[torch.nn.Parameter(torch.zeros(1))]).defaults
        self._lr0, self._lr_now, self._adam_steps = float(d["lr"]), float(d["lr"]), 0
        self._set_hyper(d, 0)
        self.gamma = gamma
        self.tmp_buffer = deque(maxlen=self.n_step)
        self.buffer_size = buffer_size
        self.memory = ReplayBuffer(buffer_size, device=self.device)
        self.run_step, self.lr_decay = run_step, lr_decay
        self._stats = torch.zeros(len(ops.MPO_STATS), dtype=torch.float32, device=self.device)
        self._noise_inject = None  # test hook of the continuous sibling: the standard normals of the next learn(), [2, num_sample, R, A], instead of torch.randn
        self._static, self._learn_graphs = None, ops.LearnGraphs("MPO.learn()")

    # what the continuous sibling answers differently at construction
    @staticmethod
    def _eligible(actor, critic, action_size, num_sample, rows):
        return actor == "discrete_policy" and critic == "discrete_q_network" and 2 <= action_size <= MAX_ACTIONS

    def _build_nets(self, R):
        """-> (actor, critic) objects for R rows; every allocation happens here, not inside a captured learn()."""
        S, A, H = self.state_size, self.action_size, self.hidden_size
        actor = ops.RainbowNet(S, A, 1, H, self.head, R, self.device, kind="pi")
        critic = ops.RainbowNet(S, A, 1, H, self.head, R, self.device, kind="q")
        critic.reserve_target_rows(2 * R)  # target(s) and target(s') share the target slot
        return actor, critic

    def _set_hyper(self, d, steps):
        for net in (self._actor, self._critic):
            net.set_hyper(d["lr"], d["betas"][0], d["betas"][1], d["eps"], steps)

    # ---------------------------------------------------------------------------------- the multipliers
    def multipliers(self):
        """ops.vmpo_block_read of the device block (synchronises)."""
        return ops.vmpo_block_read(self._mult)

    eta = property(lambda self: self.multipliers()["eta"]["value"])
    alpha_mu = property(lambda self: self.multipliers()["alpha_mu"]["value"])
    alpha_sigma = property(lambda self: self.multipliers()["alpha_sigma"]["value"])

    # ---------------------------------------------------------------------------------- acting
    @torch.no_grad()
    def act(self, state, training=True):
        """mpo.py:158-181, discrete branch; `prob` is each row's own pi[action]."""
        self.actor.train(training)
        pi = torch.softmax(self.actor(self.as_tensor(state)), dim=-1)
        action = torch.multinomial(pi, 1) if training else torch.argmax(pi, dim=-1, keepdim=True)
        prob = pi.gather(1, action)
        return {"action": action.cpu().numpy(), "prob": prob.cpu().numpy()}

    def interact_callback(self, transition):
        """mpo.py:477-484: a sliding window of n_step transitions, every key stacked on axis 1; not reset at episode ends."""
        _transition = {}
        self.tmp_buffer.append(transition)
        if len(self.tmp_buffer) == self.n_step:
            for key in self.tmp_buffer[0].keys():
                _transition[key] = np.stack([t[key] for t in self.tmp_buffer], axis=1)
        return _transition

    # ---------------------------------------------------------------------------------- learn
    def learning_rate_decay(self, step, optimizers=None, mode="cosine"):
        """base.py:93-111 on both optimizers; the multipliers follow the actor's block, which the loss kernel reads."""
        self._lr_now = self._lr0 * float(self._lr_weight(step, mode))
        self._actor.set_lr(self._lr_now)  # device scalars: the captured graph reads them
        self._critic.set_lr(self._lr_now)

    def _alloc_static(self):
        """Fixed-address buffers of one learn(): the sampled rows, the gathered batch as one [s; s'] block, the six outputs, the two gradients."""
        B, R, A = self.batch_size, self.batch_size * self.n_step, self.action_size
        idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        probe = self.memory.gather(idx, as_float=True)
        for key in ("state", "action", "reward", "next_state", "done", "prob"):
            if key not in probe:
                raise KeyError(f"MPO.learn(): the replay has no column {key!r} (act() returns 'prob'; interact_callback stacks the window)")
        if int(probe["state"].numel()) != R * self.state_size:
            raise ValueError(f"MPO.learn(): stored trajectories are {tuple(probe['state'].shape[1:])} per row, expected ({self.n_step}, {self.state_size})")
        x_all = torch.empty(2 * R, self.state_size, dtype=torch.float32, device=self.device)
        tr = dict(probe)
        tr["state"], tr["next_state"] = x_all[:R], x_all[R:]
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)
        return dict(idx=idx, tr=tr, store=self.memory._store, x_all=x_all, la=f(3, R, A, 1), lq=f(3, R, A, 1), g_la=f(R, A), g_q=f(R, A))

    def _learn_body(self, st):
        R, A = self.batch_size * self.n_step, self.action_size
        tr = self.memory.gather(st["idx"], as_float=True, out=st["tr"])
        la = self._actor.learn_forward_p(st["x_all"], R, None, st["la"])   # online(s), online(s'), target(s) in shared launches
        lq = self._critic.learn_forward_m(st["x_all"], R, None, st["lq"])  # online(s), target(s), target(s')
        g_la, g_q, _ = ops.mpo_loss_discrete(la[0].view(R, A), la[1].view(R, A), la[2].view(R, A), lq[0].view(R, A), lq[1].view(R, A), lq[2].view(R, A),
                                             tr["action"], tr["reward"], tr["done"], tr["prob"], self.n_step, self._mult, self._actor.hyper_ptr(), self.gamma,
                                             retrace=self.critic_loss_type == "retrace", stats=self._stats, out=(st["g_la"], st["g_q"]))
        self._actor.backward(g_la)
        self._critic.backward(g_q)
        self._actor.optim_step("adam", self.clip_grad_norm)  # advances the step count the NEXT learn's multiplier step reads
        self._critic.optim_step("adam", self.clip_grad_norm)

    def _run_learn(self):
        """Sample on the host (eager), then the body: eagerly the first time, captured into a hipGraph the second, replayed after (ops.LearnGraphs)."""
        if self.grad_sync is not None:
            raise NotImplementedError(MPO_ELIGIBLE)
        if self._static is None or self._static["store"] is not self.memory._store:
            self._static = self._alloc_static()
            self.reset_graphs()
        st = self._static
        self.memory.flush()
        self._draw(st)
        self._learn_graphs.run("learn", lambda: self._learn_body(st), self.use_graph)
        self.num_learn += 1
        self._adam_steps += 1

    def _draw(self, st):
        """The host side of one learn(), in front of the (replayed) body: the sampled rows."""
        st["idx"].copy_(h2d_small(self.memory.sample_indices(self.batch_size).astype(np.int64), self.device))

    def _result(self):
        s = self._read_stats(self._stats)[0]
        return {k: float(s[j]) for j, k in enumerate(ops.MPO_STATS)}

    def learn(self):
        self._run_learn()
        return self._result()

    def update_target(self):
        self._actor.sync_target()
        self._critic.sync_target()

    def process(self, transitions, step):
        """mpo.py:447-463."""
        result = {}
        if transitions:
            self.memory.store(transitions)
        self.time_t = step
        if self.memory.size >= self.batch_size and self.time_t >= self.start_train_step:
            for _ in range(self.n_epoch):
                self._run_learn()
                if self.lr_decay:
                    self.learning_rate_decay(step)
            self.update_target()
            if self.n_epoch > 0:
                result = self._result()  # the last learn's, as the reference returns; one read-back per process()
        return result

    # ---------------------------------------------------------------------------------- checkpoint, sync
    def sync_in(self, weights):
        self.actor.load_state_dict(weights)

    def sync_out(self, device="cpu"):
        return {"weights": {k: v.to(device) for k, v in self.actor.state_dict().items()}}

    def _shadows(self):
        """(ckpt key, net, shadow_of(net)) of both optimizers: the actor's also holds the three multipliers (mpo.py:142-149)."""
        mult = [torch.tensor(float(v), device=self.device) for v in self._mult[:3].tolist()]
        return [(key, net, shadow_of(net, self._optim_config, self._lr_now, extra))
                for key, net, extra in (("actor_optimizer", self._actor, mult), ("critic_optimizer", self._critic, ()))]

    def save(self, path):
        print(f"...Save model to {path}...")
        ck = {"actor": self.actor.state_dict(), "critic": self.critic.state_dict()}
        mult_m, mult_v = ops.vmpo_block_moments(self._mult)  # None where a multiplier has no optimizer state, as in torch's own: alpha_sigma of a discrete policy never steps
        for key, net, (opt, params, keys) in self._shadows():
            if self._adam_steps > 0:
                m, v = moments_of(net)
                optim_state.fill(opt, params, self._adam_steps, m + mult_m, v + mult_v)  # (zip: the critic's ends at its own parameters)
            ck[key] = opt.state_dict()
        torch.save(ck, os.path.join(path, "ckpt"))

    def load(self, path):
        print(f"...Load model from {path}...")
        ck = torch.load(os.path.join(path, "ckpt"), map_location=self.device, weights_only=False)
        for view, target, key in ((self.actor, self.target_actor, "actor"), (self.critic, self.target_critic, "critic")):
            view.load_state_dict(ck[key])
            target.load_state_dict(ck[key])
        steps, g0 = 0, None
        for key, net, (opt, params, keys) in self._shadows():
            opt.load_state_dict(ck[key])
            steps = load_moments(net, keys, opt, params) or steps
            if len(params) > len(keys):  # the multipliers' moments go into the block; their VALUES are not in the reference's checkpoint and stay
                _, m, v = optim_state.read(opt, params[len(keys):])
                ops.vmpo_block_set_moments(self._mult, m, v)
            g0 = g0 or opt.param_groups[0]
        self._adam_steps, self._lr_now = steps, float(g0["lr"])
        self._set_hyper(g0, steps)

    def _resume_extra_attrs(self):
        return {"mpo_block": ops.vmpo_block_hex(self._mult)}

    def _resume_load_extra_attrs(self, d):
        if "mpo_block" in d:
            ops.vmpo_block_from_hex(self._mult, d["mpo_block"])


class _SampledCritic:
    """The one critic of an ops.ACNet (continuous_q_network with its target, jh_acnet_*) behind the bucket surface MPO's code uses of an
    ops.RainbowNet: params / target / grads / m / v, export_state / import_state by bucket, set_hyper / set_lr / sync_target.  The object's
    deterministic actor stays idle: never imported, exported or stepped."""

    def __init__(self, state_size, action_size, hidden_size, rows, sampled_rows, device):
        self.nat = ops.ACNet(state_size, action_size, hidden_size, 1, rows, device)
        self.nat.reserve_sampled(sampled_rows)  # allocated here, not inside a captured learn()
        self.device = self.nat.device
        self.params, self.target, self.grads, self.m, self.v = (self.nat.critics[k] for k in self.nat.KINDS)

    def _kind(self, bucket):
        return "params" if bucket is None else next(k for k in self.nat.KINDS if self.nat.critics[k] is bucket)

    def export_state(self, bucket=None):
        return self.nat.export_state("critic", self._kind(bucket))

    def import_state(self, sd, bucket=None):
        self.nat.import_state(sd, "critic", self._kind(bucket))

    def set_hyper(self, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=0):
        self.nat.set_hyper("critic", lr, beta1, beta2, eps, step)

    def set_lr(self, lr):
        self.nat.set_lr("critic", lr)

    def sync_target(self):
        self.nat.sync_target()


class MPOContinuous(MPO):
    """core/agent/mpo.py:14-484 for a continuous policy: Agent("mpo", actor="continuous_policy", critic="continuous_q_network").  What differs
    from the discrete class above:

      networks      the actor is the Gaussian policy (ops.RainbowNet kind "gauss": raw [mu | log_std] rows), the critic a continuous Q-network
                    in an ops.ACNet with one critic (_SampledCritic); the reference's construction order, so one torch.manual_seed gives its weights.
      learn()       gather -> the actor's online(s), online(s'), target(s) -> jh_mpo_sample (num_sample actions per row from online(s') and from
                    target(s)) -> ALL critic forwards in five grouped launches (jh_acnet_mpo_forward: head.l(s) once per state row, not once per
                    sample) -> jh_mpo_loss_continuous (Retrace, the E-step over the samples, the Gaussian M-step and trust region, all THREE
                    multipliers' steps) -> the actor's backward and clip + Adam -> the critic's (jh_acnet_critic_fit).  One hipGraph.
      noise         the 2 x num_sample x R x A standard normals of a learn() are torch.randn into a static buffer in front of the replay, as SAC
                    draws its own; `_noise_inject` [2, N, R, A] replaces them (tests).  torch's own stream for Normal.sample is not reproduced.
      act()         the reference's continuous branch in torch on the native actor's raw heads: prob = exp(sum log_prob(z)), z = mu in evaluation."""

    action_type = "continuous"

    @staticmethod
    def _eligible(actor, critic, action_size, num_sample, rows):
        return (actor == "continuous_policy" and critic == "continuous_q_network" and 1 <= action_size <= ops.MPO_MAX_CONT_ACTIONS
                and isinstance(num_sample, (int, np.integer)) and num_sample >= 1 and num_sample * rows <= ops.MPO_MAX_SAMPLED)

    def _build_nets(self, R):
        S, A, H = self.state_size, self.action_size, self.hidden_size
        self.num_sample = int(self.num_sample)
        return ops.RainbowNet(S, A, 1, H, self.head, R, self.device, kind="gauss"), _SampledCritic(S, A, H, R, self.num_sample * R, self.device)

    @staticmethod
    def _policy(raw, A):
        """network/policy.py:53-55 on the raw heads [rows, 2A] -> (mu, std)"""
        return torch.clamp(raw[:, :A], min=-5.0, max=5.0), torch.tanh(raw[:, A:]).exp()

    @torch.no_grad()
    def act(self, state, training=True):
        """mpo.py:160-167."""
        self.actor.train(training)
        mu, std = self._policy(self.actor(self.as_tensor(state)), self.action_size)
        m = torch.distributions.Normal(mu, std)
        z = m.sample() if training else mu
        prob = m.log_prob(z).sum(axis=-1, keepdims=True).exp()
        return {"action": torch.tanh(z).cpu().numpy(), "prob": prob.cpu().numpy()}

    def _alloc_static(self):
        """MPO._alloc_static's gathered batch, then the fixed-address buffers of the continuous body: the three raw heads, the normals, the
        sampled z and actions, the four critic outputs, the two gradients."""
        B, R, A, N = self.batch_size, self.batch_size * self.n_step, self.action_size, self.num_sample
        idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        probe = self.memory.gather(idx, as_float=True)
        for key in ("state", "action", "reward", "next_state", "done", "prob"):
            if key not in probe:
                raise KeyError(f"MPO.learn(): the replay has no column {key!r} (act() returns 'prob'; interact_callback stacks the window)")
        if int(probe["state"].numel()) != R * self.state_size or int(probe["action"].numel()) != R * A:
            raise ValueError(f"MPO.learn(): stored trajectories are state {tuple(probe['state'].shape[1:])} / action {tuple(probe['action'].shape[1:])} per row, "
                             f"expected ({self.n_step}, {self.state_size}) / ({self.n_step}, {A})")
        x_all = torch.empty(2 * R, self.state_size, dtype=torch.float32, device=self.device)
        tr = dict(probe)
        tr["state"], tr["next_state"] = x_all[:R], x_all[R:]
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
        return dict(idx=idx, tr=tr, store=self.memory._store, x_all=x_all, la=f(3, R, 2 * A, 1), eps=f(2, N, R, A), z=f(2, N, R, A), a=f(2, N, R, A),
                    lq=(f(R), f(R), f(N, R), f(N, R)), g_la=f(R, 2 * A), g_q=f(R))

    def _draw(self, st):
        """The sampled rows, then the normals of this learn()'s two Normal.sample calls (mpo.py:223, 255; online(s') first), eagerly into the
        static buffer the captured body reads: a replayed graph sees fresh draws."""
        super()._draw(st)
        if self._noise_inject is not None:
            st["eps"].copy_(torch.as_tensor(self._noise_inject).to(self.device, torch.float32).reshape(st["eps"].shape))
        else:
            torch.randn(st["eps"].shape, out=st["eps"])

    def _learn_body(self, st):
        R, A = self.batch_size * self.n_step, self.action_size
        tr = self.memory.gather(st["idx"], as_float=True, out=st["tr"])
        la = self._actor.learn_forward_p(st["x_all"], R, None, st["la"]).view(3, R, 2 * A)  # online(s), online(s'), target(s), raw
        zn, zt_add, a_next, a_add = ops.mpo_sample(la[1], la[2], st["eps"], out=(st["z"], st["a"]))
        q, qt_a, qt_next, qt_add = self._critic.nat.mpo_forward(st["x_all"], tr["action"], a_next, a_add, out=st["lq"])
        g_la, g_q, _ = ops.mpo_loss_continuous(la[0], la[2], q, qt_a, qt_next, qt_add, zt_add, tr["action"], tr["reward"], tr["done"], tr["prob"], self.n_step,
                                               self._mult, self._actor.hyper_ptr(), self.gamma, retrace=self.critic_loss_type == "retrace", stats=self._stats,
                                               out=(st["g_la"], st["g_q"]))
        self._actor.backward(g_la)
        self._actor.optim_step("adam", self.clip_grad_norm)  # advances the step count the NEXT learn's multiplier step reads
        self._critic.nat.critic_fit(st["x_all"][:R], tr["action"], g_q, self.clip_grad_norm)
