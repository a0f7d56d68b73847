import os

import numpy as np
import torch

from ... import ops
from ..buffer import ReplayBuffer
from ..network import Network
from . import optim_state
from .base import BaseAgent

_ELIGIBLE = ("{name} runs on libjorldy_hip only: actor 'deterministic_policy', critic 'continuous_q_network', head 'mlp' with a scalar state_size, "
             "hidden_size % 4 == 0, action_size >= 1, optim_config {{'actor': 'adam', 'critic': 'adam', actor_lr, critic_lr}} ({configs} and their shapes); "
             "the cnn head is not on the native engine")
TD3_ELIGIBLE = _ELIGIBLE.format(name="TD3", configs="config.td3 x mujoco / cartpole")


class ActorCriticView:
    """`agent.actor`, `agent.critic1`, `agent.target_actor`, ... as the reference's modules are used: callable, state_dict in the reference's
    keys, on top of ops.ACNet's flat buckets.  net: "actor" | "critic1" | "critic2"; which: 0 online / 1 target."""

    def __init__(self, acnet, net, which):
        self._net, self._name, self._which, self.training = acnet, net, which, True

    def _kind(self):
        return "params" if self._which == 0 else "target"

    def state_dict(self):
        return self._net.export_state(self._name, self._kind())

    def load_state_dict(self, sd, strict=True):
        self._net.import_state(sd, self._name, self._kind())

    def parameters(self):
        return list(self.state_dict().values())

    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def to(self, *args, **kwargs):
        return self

    @torch.no_grad()
    def __call__(self, x, action=None):
        net = self._net
        x = x.contiguous()
        outs = []
        for o in range(0, x.shape[0], net.maxB):
            xs = x[o : o + net.maxB]
            if self._name == "actor":
                outs.append(net.actor_forward(xs, self._which))
            else:
                c = 1 if self._name == "critic2" else 0
                outs.append(net.critic_forward(xs, action[o : o + net.maxB].contiguous(), self._which)[c].reshape(-1, 1))
        return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


class DeterministicActorCritic(BaseAgent):
    """What TD3 and DDPG share: the network object (ops.ACNet, jh_acnet_*), the replay store and gather, learn() as a critic update
    [+ actor update [+ soft update]] captured into one hipGraph per variant, mapped statistics, the reference's checkpoint format."""

    action_type = "continuous"
    N_CRITICS = 2
    TARGET_NOISE = True  # learn() draws [B, A] standard normals for the target action; False: the target action is plain tanh (DDPG)
    target_noise_std = target_noise_clip = 0.0  # what the critic update scales and clips that noise with; a subclass with TARGET_NOISE sets them
    ELIGIBLE = TD3_ELIGIBLE
    # the reference's save_dict in its own order: (key in the ckpt, network, "net" | "opt")
    CKPT_KEYS = (("actor", "actor", "net"), ("actor_optimizer", "actor", "opt"), ("critic1", "critic1", "net"), ("critic2", "critic2", "net"),
                 ("critic_optimizer1", "critic1", "opt"), ("critic_optimizer2", "critic2", "opt"))  # td3.py:232-239
    _RESUME_ATTRS = BaseAgent._RESUME_ATTRS + ("num_random_step", "actor_loss", "_adam_steps_actor", "_adam_steps_critic")

    # what a member of the family sets: its policy module and the view `agent.actor` is, the optimizers optim_config may name, the actor's
    # default lr, the floats of the mapped statistics and where in them the actor update leaves its arrival mark
    ACTOR, ACTOR_VIEW, OPTIMIZERS, ACTOR_LR, N_STATS, ACTOR_MARK = "deterministic_policy", ActorCriticView, ("actor", "critic"), 1e-3, 8, 5

    def _make_net(self, state_size, action_size, hidden_size, batch_size):
        return ops.ACNet(state_size, action_size, hidden_size, self.N_CRITICS, batch_size, self.device)

    def _init_common(self, state_size, action_size, hidden_size, actor, critic, head, optim_config, gamma, buffer_size, batch_size, start_train_step, tau,
                     run_step, lr_decay, device, use_graph, build_order):
        got = (f"; got actor={actor!r}, critic={critic!r}, head={head!r}, state_size={state_size!r}, action_size={action_size!r}, hidden_size={hidden_size!r}, "
               f"optim_config={optim_config!r}")
        ok_opt = (isinstance(optim_config, dict) and set(optim_config) <= {o + s for o in self.OPTIMIZERS for s in ("", "_lr")}
                  and all(str(optim_config.get(o, "adam")).lower() == "adam" for o in self.OPTIMIZERS))
        ok = (actor == self.ACTOR and critic == "continuous_q_network" and head == "mlp" and np.isscalar(state_size) and np.isscalar(action_size)
              and int(action_size) >= 1 and isinstance(hidden_size, (int, np.integer)) and hidden_size % 4 == 0 and ok_opt)
        if not ok:
            raise ValueError(self.ELIGIBLE + got)
        self.device = self._require_gpu(device)
        self.use_graph = use_graph
        self.grad_sync = None
        self.state_size, self.action_size = int(state_size), int(action_size)
        self._net = self._make_net(state_size, action_size, hidden_size, batch_size)
        # the reference's construction order: every module, the targets included, draws its initial weights from torch's generator (a target
        # is then overwritten by its online net); each becomes `self.<net>` / `self.target_<net>`
        for name in build_order:
            kind, net = name.split(":")
            mod = Network(actor if net == "actor" else critic, state_size, action_size, D_hidden=hidden_size, head=head)
            if kind == "online":
                self._net.import_state(mod.state_dict(), net)
                setattr(self, net, (self.ACTOR_VIEW if net == "actor" else ActorCriticView)(self._net, net, 0))
            else:
                setattr(self, "target_" + net, ActorCriticView(self._net, net, 1))
        self._net.sync_target()  # target.load_state_dict(online.state_dict())
        self.network = self.actor  # BaseAgent.sync_in / sync_out carry the actor only (td3.py:255-265, sac.py:345-352)
        self._lr0 = {"actor": float(optim_config.get("actor_lr", self.ACTOR_LR)), "critic": float(optim_config.get("critic_lr", 1e-3))}
        self._lr_now = dict(self._lr0)
        self._adam_steps_actor = self._adam_steps_critic = 0
        for which in ("actor", "critic"):
            self._net.set_hyper(which, self._lr0[which], 0.9, 0.999, 1e-8, 0)
        self.gamma, self.tau = gamma, tau
        self.buffer_size = buffer_size
        self.memory = ReplayBuffer(buffer_size, device=self.device)
        self.memory.defer_rows = 16  # per-step stores coalesce into one ring append before the next learn()
        self.batch_size = batch_size
        self.start_train_step = start_train_step
        self.num_learn = 0
        self.time_t = 0
        self.run_step = run_step
        self.lr_decay = lr_decay
        self._noise_inject = None  # test hook: the standard normals of the next learn() ([B, A]; SAC [2, B, A]) instead of torch.randn
        self._stats = self._mapped_stats(self.N_STATS)  # critic: loss_1, loss_2, max_Q, mark; then the actor update's, its mark last
        self._static, self._learn_graphs = None, ops.LearnGraphs(f"{type(self).__name__}.learn()")

    # ------------------------------------------------------------------------------------------ acting
    @torch.no_grad()
    def _actor_np(self, state):
        return self.actor(self.as_tensor(state)).cpu().numpy()

    # ------------------------------------------------------------------------------------------ learning
    def _alloc_static(self):
        B, A = self.batch_size, self.action_size
        idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        probe = self.memory.gather(idx, idx_offset=0, as_float=True)
        x_all = torch.empty((2 * B,) + tuple(probe["state"].shape[1:]), dtype=torch.float32, device=self.device)
        tr = dict(probe)
        tr["state"], tr["next_state"] = x_all[:B], x_all[B:]  # one contiguous [state; next_state] batch
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)
        return dict(idx=idx, tr=tr, store=self.memory._store, x_all=x_all, noise=f(B, A), y=f(B), q=f(self.N_CRITICS, B), a_pred=f(B, A))

    def _draw(self, st):
        """Host side of sampling (the reference's numpy draw), then the target noise of this learn() (td3.py:159: torch.randn_like(action)),
        eagerly into the static buffer the captured body reads: a replayed graph sees fresh draws."""
        from ..buffer.base import h2d_small

        st["idx"].copy_(h2d_small(self.memory.sample_indices(self.batch_size).astype(np.int64), self.device))
        if not self.TARGET_NOISE:
            return
        if self._noise_inject is not None:
            st["noise"].copy_(torch.as_tensor(self._noise_inject).to(self.device, torch.float32).reshape(st["noise"].shape))
        else:
            torch.randn(st["noise"].shape, out=st["noise"])

    def _learn_body(self, st, actor_step, soft):
        B, net = self.batch_size, self._net
        tr = self.memory.gather(st["idx"], as_float=True, out=st["tr"])
        net.critic_update(st["x_all"], tr["action"], tr["reward"], tr["done"], st["noise"] if self.TARGET_NOISE else None, self.gamma,
                          self.target_noise_std, self.target_noise_clip, self._stats.dev, y=st["y"], q=st["q"])
        if actor_step:
            net.actor_update(st["x_all"][:B], self._stats.dev[4:6], action_pred=st["a_pred"])
        if soft:
            net.soft_update(self.tau)

    def _run_learn(self, actor_step, soft, capture):
        """Sample on the host (eager), then run the body: eagerly the first time (and whenever `capture` is off for this variant), captured
        into a hipGraph of its own per variant on first use after that, replayed from then on."""
        if self._static is None or self._static["store"] is not self.memory._store:
            self._static = self._alloc_static()
            self.reset_graphs()
        st = self._static
        self.memory.flush()
        self._draw(st)
        # one graph per variant; the variants share one warm-up (the first learn() of any of them)
        self._learn_graphs.run((actor_step, soft), lambda: self._learn_body(st, actor_step, soft), self.use_graph and capture, warm_key="learn")
        self._adam_steps_critic += 1
        self._adam_steps_actor += int(actor_step)

    def _learn_stats(self, actor_step, soft, capture=True):
        marks = (3, self.ACTOR_MARK) if actor_step else (3,)
        self._stats.arm(marks)
        self._run_learn(actor_step, soft, capture)
        self._stats.wait(marks, type(self).__name__ + ".learn(): the statistics")
        return self._stats.np.copy()

    def learning_rate_decay(self, step, optimizers=None, mode="cosine"):
        """base.py:93-111 on the actor's and the critics' optimizers: one weight for both (td3.py:219-226)."""
        w = float(self._lr_weight(step, mode))
        for which in ("actor", "critic"):
            self._lr_now[which] = self._lr0[which] * w
            self._net.set_lr(which, self._lr_now[which])  # a device scalar: the captured graphs read it

    def update_target_soft(self):
        self._net.soft_update(self.tau)

    def _store(self, transitions):
        if isinstance(transitions, dict):
            self.memory.store_soa(transitions)
        else:
            self.memory.store(transitions)

    # ------------------------------------------------------------------------------------------ checkpoints
    def _critic_names(self):
        return self._net.nets()[1:]

    def _ckpt(self):
        out = {}
        for key, net, what in self.CKPT_KEYS:
            sd = self._net.export_state(net)
            if what == "net":
                out[key] = sd
                continue
            steps, lr = (self._adam_steps_actor, self._lr_now["actor"]) if net == "actor" else (self._adam_steps_critic, self._lr_now["critic"])
            opt, params = optim_state.shadow({"name": "adam"}, sd.values(), lr)
            if steps > 0:
                optim_state.fill(opt, params, steps, *(list(self._net.export_state(net, kind).values()) for kind in "mv"))
            out[key] = opt.state_dict()
        return out

    def save(self, path):
        print(f"...Save model to {path}...")
        torch.save(self._ckpt(), os.path.join(path, "ckpt"))

    def load(self, path):
        """The reference's ckpt, with two deliberate departures: critic 2 is restored from "critic2" (td3.py:249 loads it into critic 1 and
        leaves critic 2 as constructed), and EVERY target equals its loaded online network afterwards (ddpg.py:191-199 leaves target_actor
        stale).  The critics share one optimizer block: critic 1's step count, lr, betas and eps hold for both."""
        print(f"...Load model from {path}...")
        self._load_ckpt(torch.load(os.path.join(path, "ckpt"), map_location=self.device, weights_only=False))

    def _load_ckpt(self, ckpt):
        for key, net, what in self.CKPT_KEYS:
            if what == "net":
                self._net.import_state(ckpt[key], net)
                continue
            sd = self._net.export_state(net)
            opt, params = optim_state.shadow({"name": "adam"}, sd.values(), 0.0)
            opt.load_state_dict(ckpt[key])
            steps, m, v = optim_state.read(opt, params)
            for kind, moments in (("m", m), ("v", v)):
                self._net.import_state(dict(zip(sd, optim_state.dense(moments, params))), net, kind)
            lr, beta1, beta2, eps, _ = optim_state.hyper(opt.param_groups[0])
            if net == "actor":
                self._adam_steps_actor, self._lr_now["actor"] = steps, lr
                self._net.set_hyper("actor", lr, beta1, beta2, eps, steps)
            elif net == "critic1":
                self._adam_steps_critic, self._lr_now["critic"] = steps, lr
                self._net.set_hyper("critic", lr, beta1, beta2, eps, steps)
        self._net.sync_target()

    # ---- complete checkpoints: BaseAgent.save_full / load_full + the targets and the exploration state
    def save_full(self, path, version=None):
        """BaseAgent's format version 2 only: the single-pickle version 1 has no place for the exploration state."""
        if version not in (None, 2):
            raise ValueError(f"{type(self).__name__}.save_full writes resume format version 2 only, got version={version!r}")
        super().save_full(path, version)
        d = os.path.join(path, "resume")
        os.makedirs(d, exist_ok=True)
        torch.save({net: self._net.export_state(net, "target") for net in self._net.nets()}, os.path.join(d, "targets.pt"))

    def load_full(self, path):
        super().load_full(path)
        f = os.path.join(path, "resume", "targets.pt")
        if os.path.exists(f):
            for net, sd in torch.load(f, map_location=self.device, weights_only=False).items():
                self._net.import_state(sd, net, "target")


class TD3(DeterministicActorCritic):
    """core/agent/td3.py:14-265: twin delayed DDPG.  Two critics trained against y = r + (1 - d) gamma min_i Q_i'(s', clamp(pi'(s') + clipped
    noise)); every `update_delay` learns the actor steps along -mean Q_1(s, pi(s)) -- backward through critic 1's action input -- and, from the
    second learn on, all three targets move by Polyak averaging.  Everything of learn() runs on libjorldy_hip (ops.ACNet, jh_acnet_*); the
    three variants of learn() (actor step without soft update: the first learn, run eagerly; critics only; actor step with soft update) are
    one hipGraph each.  Unknown keywords are swallowed as in the reference (config.td3.cartpole passes actor_period / act_noise_std, which
    nobody reads)."""

    def __init__(self, state_size, action_size, hidden_size=256, actor="deterministic_policy", critic="continuous_q_network", head="mlp",
                 optim_config={"actor": "adam", "critic": "adam", "actor_lr": 1e-3, "critic_lr": 1e-3}, gamma=0.99, buffer_size=50000, batch_size=128,
                 start_train_step=1000, initial_random_step=0, tau=1e-3, update_delay=2, action_noise_std=0.1, target_noise_std=0.2, target_noise_clip=0.5,
                 run_step=1e6, lr_decay=True, device=None, use_graph=True, **kwargs):
        self._init_common(state_size, action_size, hidden_size, actor, critic, head, optim_config, gamma, buffer_size, batch_size, start_train_step, tau, run_step,
                          lr_decay, device, use_graph,
                          ("online:actor", "target:actor", "online:critic1", "target:critic1", "online:critic2", "target:critic2"))  # td3.py:77-112
        self.actor_loss = 0.0
        self.initial_random_step = initial_random_step
        self.num_random_step = 0
        self.update_delay = update_delay
        self.action_noise_std = action_noise_std
        self.target_noise_std = target_noise_std
        self.target_noise_clip = target_noise_clip

    @torch.no_grad()
    def act(self, state, training=True):
        """td3.py:132-144: uniform actions [1, A] (whatever the number of rows) during the random phase; otherwise the actor plus ONE normal
        vector for all rows, clipped to +-1; no noise in evaluation."""
        self.actor.train(training)
        if training and self.num_random_step < self.initial_random_step:
            action = np.random.uniform(-1.0, 1.0, (1, self.action_size))
            self.num_random_step += 1
        else:
            action = self._actor_np(state)
            if training:
                noise = np.random.normal(0, self.action_noise_std, self.action_size)
                action = (action + noise).clip(-1.0, 1.0)
        return {"action": action}

    def learn(self):
        actor_step = self.num_learn % self.update_delay == 0  # td3.py:181
        soft = actor_step and self.num_learn > 0              # td3.py:189
        s = self._learn_stats(actor_step, soft, capture=not (actor_step and not soft))
        if actor_step:
            self.actor_loss = float(s[4])
        self.num_learn += 1
        self.result = {"critic_loss1": float(s[0]), "critic_loss2": float(s[1]), "actor_loss": self.actor_loss, "max_Q": float(s[2])}
        return self.result

    def process(self, transitions, step):
        """td3.py:211-228."""
        result = {}
        self._store(transitions)
        self.time_t = step
        if self.memory.size >= self.batch_size and step >= self.start_train_step:
            result = self.learn()
            if self.lr_decay:
                self.learning_rate_decay(step)
        return result
