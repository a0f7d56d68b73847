import os

import numpy as np
import torch

from ... import ops
from ..buffer import ReplayBuffer
from ..network import Network
from . import optim_state
from .base import BaseAgent
from .native_net import NativeNet, load_moments, moments_of, shadow_of
from .td3 import ActorCriticView, DeterministicActorCritic

SAC_ELIGIBLE = ("SAC runs on libjorldy_hip only: actor 'continuous_policy', critic 'continuous_q_network', head 'mlp' with a scalar state_size, "
                "hidden_size % 4 == 0, action_size >= 1, optim_config {'actor': 'adam', 'critic': 'adam', 'alpha': 'adam', actor_lr, critic_lr, alpha_lr} "
                "(config.sac x mujoco / pendulum / cartpole / hopper_mlagent and their shapes); or the discrete SAC: actor 'discrete_policy' together "
                f"with critic 'discrete_q_network' under the same head, hidden_size and optimizer rules at 2 <= action_size <= {ops.SACD_MAX_ACTIONS} and "
                f"batch_size <= {ops.SACD_MAX_ROWS} < buffer_size (process() learns only with more stored rows than one batch: a smaller replay never learns) and a GPU device "
                "(config.sac x cartpole_discrete / pong_mlagent and their shapes); a discrete actor with a continuous "
                "critic, or the reverse, is refused; the cnn head and data-parallel learners (grad_sync) are not on the native engine")


class GaussianActorView(ActorCriticView):
    """`agent.actor` as the reference's ContinuousPolicy is used: actor(x) -> (mu, std)."""

    @torch.no_grad()
    def __call__(self, x):
        net = self._net
        x = x.contiguous()
        outs = [net.actor_forward(x[o : o + net.maxB]) for o in range(0, x.shape[0], net.maxB)]
        return outs[0] if len(outs) == 1 else tuple(torch.cat(p, 0) for p in zip(*outs))


class SAC(DeterministicActorCritic):
    """core/agent/sac.py:14-352, continuous actions: a Gaussian actor (online only), two critics trained against
    y = r + (1 - d) gamma (min_i Q_i'(s', a') - alpha logp(a')) with a' from the ONLINE actor, an actor step through both critics' action
    inputs and through logp, and a temperature alpha = exp(log_alpha) that is either static or follows its own one-parameter Adam.  All of
    learn() runs on libjorldy_hip (ops.SACNet, jh_sacnet_*) as one body -- critic update, actor update with the temperature's bookkeeping in
    its seed kernel -- captured into one hipGraph after an eager warm-up; process() replays the variant that ends with the soft update of the
    two target critics.  The two [B, A] normal draws of a learn() are torch.randn into static buffers before the replay, the target's first.
    The temperature lives on the device: the alpha of learn k is exp(log_alpha) after k - 1 Adam steps (sac.py:250-255 refreshes it after
    the actor step and steps log_alpha after that).  Unknown keywords are swallowed as in the reference (target_update_period is accepted
    and unused for the continuous agent)."""

    ELIGIBLE = SAC_ELIGIBLE
    _RESUME_ATTRS = BaseAgent._RESUME_ATTRS + ("_adam_steps_actor", "_adam_steps_critic")
    # the stats after the critic's four: actor_loss, alpha_loss, mean_Q, alpha, entropy, mark
    ACTOR, ACTOR_VIEW, OPTIMIZERS, ACTOR_LR, N_STATS, ACTOR_MARK = "continuous_policy", GaussianActorView, ("actor", "critic", "alpha"), 5e-4, 12, 9
    RESULT_KEYS = ("critic_loss1", "critic_loss2", "max_Q", None, "actor_loss", "alpha_loss", "mean_Q", "alpha", "entropy")

    def __new__(cls, state_size=None, action_size=None, hidden_size=512, actor="continuous_policy", critic="continuous_q_network", *args, **kwargs):
        """Agent("sac", actor="discrete_policy", critic="discrete_q_network", ...) is the sibling class below (a mixed pair too: it refuses it);
        everything else, refusals included, is this one."""
        discrete = str(actor).startswith("discrete") or str(critic).startswith("discrete")
        return object.__new__(SACDiscrete if cls is SAC and discrete else cls)

    def __init__(self, state_size, action_size, hidden_size=512, actor="continuous_policy", critic="continuous_q_network", head="mlp",
                 optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}, use_dynamic_alpha=False,
                 gamma=0.99, tau=5e-3, buffer_size=50000, batch_size=64, start_train_step=2000, static_log_alpha=-2.0, target_update_period=10000, run_step=1e6,
                 lr_decay=True, device=None, use_graph=True, **kwargs):
        self._init_common(state_size, action_size, hidden_size, actor, critic, head, optim_config, gamma, buffer_size, batch_size, start_train_step, tau, run_step,
                          lr_decay, device, use_graph, ("online:actor", "online:critic1", "target:critic1", "online:critic2", "target:critic2"))  # sac.py:75-95
        self.use_dynamic_alpha = bool(use_dynamic_alpha)
        self.alpha_lr = float(optim_config.get("alpha_lr", 3e-4))  # never decayed (sac.py:292-300)
        self._net.set_alpha(0.0 if self.use_dynamic_alpha else static_log_alpha, lr=self.alpha_lr, dynamic=self.use_dynamic_alpha)
        self.target_entropy = -self.action_size
        self.target_update_stamp = 0
        self.target_update_period = target_update_period

    def _make_net(self, state_size, action_size, hidden_size, batch_size):
        return ops.SACNet(state_size, action_size, hidden_size, batch_size, self.device)

    # ------------------------------------------------------------------------------------------ the temperature
    @property
    def log_alpha(self):
        return self._net.get_alpha()["log_alpha"]

    @property
    def alpha(self):
        """The alpha the next learn() forms its losses with."""
        return self._net.get_alpha()["alpha"]

    # ------------------------------------------------------------------------------------------ acting
    @torch.no_grad()
    def act(self, state, training=True):
        """sac.py:143-159: tanh of a draw from Normal(mu, std) -- torch.normal on the device's generator -- or tanh(mu) in evaluation."""
        self.actor.train(training)
        mu, std = self.actor(self.as_tensor(state))
        z = torch.normal(mu, std) if training else mu
        return {"action": torch.tanh(z).cpu().numpy()}

    # ------------------------------------------------------------------------------------------ learning
    def _alloc_static(self):
        st = super()._alloc_static()
        B, A = self.batch_size, self.action_size
        f = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=self.device)
        st.update(noise=f(2, B, A), a_next=f(B, A), logp_next=f(B), logp=f(B), q_pi=f(2, B))
        return st

    def _draw(self, st):
        """Host side of sampling (the reference's numpy draw), then the two normal draws of this learn() (sac.py:163 via 188 and 230), eagerly into
        the static buffer the captured body reads: a replayed graph sees fresh draws."""
        from ..buffer.base import h2d_small

        st["idx"].copy_(h2d_small(self.memory.sample_indices(self.batch_size).astype(np.int64), self.device))
        if self._noise_inject is not None:
            st["noise"].copy_(torch.as_tensor(self._noise_inject).to(self.device, torch.float32).reshape(st["noise"].shape))
        else:
            torch.randn(st["noise"][0].shape, out=st["noise"][0])
            torch.randn(st["noise"][1].shape, out=st["noise"][1])

    def _learn_body(self, st, actor_step, soft):
        B, net = self.batch_size, self._net
        tr = self.memory.gather(st["idx"], as_float=True, out=st["tr"])
        net.critic_update(st["x_all"], tr["action"], tr["reward"], tr["done"], st["noise"][0], self.gamma, self._stats.dev, y=st["y"], q=st["q"], a_next=st["a_next"],
                          logp_next=st["logp_next"])
        net.actor_update(st["x_all"][:B], st["noise"][1], self._stats.dev[4:10], action=st["a_pred"], logp=st["logp"], q=st["q_pi"])
        if soft:
            net.soft_update(self.tau)

    def _learn(self, soft):
        s = self._learn_stats(True, soft)
        self.num_learn += 1
        self.result = {k: float(s[i]) for i, k in enumerate(self.RESULT_KEYS) if k is not None}
        return self.result

    def learn(self):
        """sac.py:171-269.  Moves no target."""
        return self._learn(False)

    def process(self, transitions, step):
        """sac.py:281-310: learns when memory.size > batch_size (strict); the lr decay touches the actor's and the critics' optimizers only;
        once learning has begun every call ends with the soft update of the two target critics -- inside the captured learn() when this call
        learns (the update reads neither learning rate, so its place before the decay changes nothing)."""
        result = {}
        self._store(transitions)
        self.target_update_stamp += step - self.time_t
        self.time_t = step
        if self.memory.size > self.batch_size and step >= self.start_train_step:
            result = self._learn(True)
            if self.lr_decay:
                self.learning_rate_decay(step)
        elif self.num_learn > 0:
            self.update_target_soft()
        return result

    # ------------------------------------------------------------------------------------------ checkpoints
    def _one(self, v):
        """The temperature's scalars as the one-element tensors of the reference's log_alpha."""
        return torch.tensor([v], dtype=torch.float32, device=self.device)

    def _ckpt(self):
        """The reference's keys (sac.py:312-326): TD3's six, plus log_alpha and alpha_optimizer when the temperature is dynamic."""
        out = super()._ckpt()
        if self.use_dynamic_alpha:
            blk = self._net.get_alpha()
            opt, params = optim_state.shadow({"name": "adam", "betas": (blk["beta1"], blk["beta2"]), "eps": blk["eps"]}, [self._one(blk["log_alpha"])], blk["lr"])
            if blk["step"] > 0:
                optim_state.fill(opt, params, blk["step"], [self._one(blk["m"])], [self._one(blk["v"])])
            out["log_alpha"], out["alpha_optimizer"] = params[0].detach(), opt.state_dict()
        return out

    def load(self, path):
        """The reference's ckpt, with three deliberate departures: critic 2 is restored from "critic2" (sac.py:335 loads it into critic 1 and
        leaves critic 2 as constructed); both targets equal their loaded online critics afterwards (the reference copies critic 2 as
        constructed); and the alpha in use becomes exp(loaded log_alpha) with the alpha optimizer's state restored (sac.py:341-343 rebinds
        log_alpha, which orphans the optimizer's parameter, and leaves self.alpha as it was until the next learn())."""
        print(f"...Load model from {path}...")
        ckpt = torch.load(os.path.join(path, "ckpt"), map_location=self.device, weights_only=False)
        self._load_ckpt(ckpt)
        if self.use_dynamic_alpha and "log_alpha" in ckpt:
            la = float(torch.as_tensor(ckpt["log_alpha"]).reshape(-1)[0])
            opt, params = optim_state.shadow({"name": "adam"}, [self._one(la)], self.alpha_lr)
            opt.load_state_dict(ckpt["alpha_optimizer"])
            steps, m, v = optim_state.read(opt, params)
            lr, beta1, beta2, eps, _ = optim_state.hyper(opt.param_groups[0])
            self._net.set_alpha(la, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=steps, m=float(optim_state.dense(m, params)[0]),
                                v=float(optim_state.dense(v, params)[0]), dynamic=True)

    def save_full(self, path, version=None):
        """BaseAgent's format version 2 only.  Beside the replay buffer, the counters and the generators it carries the two target critics and
        the whole temperature block (log_alpha, the alpha in use, Adam's moments and step count): a resumed run continues bit for bit."""
        if version not in (None, 2):
            raise ValueError(f"SAC.save_full writes resume format version 2 only, got version={version!r}")
        super(DeterministicActorCritic, self).save_full(path, version)
        d = os.path.join(path, "resume")
        os.makedirs(d, exist_ok=True)
        torch.save({net: self._net.export_state(net, "target") for net in self._critic_names()}, os.path.join(d, "targets.pt"))
        torch.save(self._net.get_alpha(), os.path.join(d, "alpha.pt"))

    def load_full(self, path):
        super().load_full(path)  # the targets: DeterministicActorCritic.load_full
        f = os.path.join(path, "resume", "alpha.pt")
        if os.path.exists(f):
            b = torch.load(f, map_location="cpu", weights_only=False)
            self._net.set_alpha(b["log_alpha"], alpha=b["alpha"], lr=b["lr"], beta1=b["beta1"], beta2=b["beta2"], eps=b["eps"], step=b["step"], m=b["m"], v=b["v"],
                                dynamic=b["dynamic"])


class SACDiscrete(SAC):
    """core/agent/sac.py:14-352 for discrete actions: Agent("sac", actor="discrete_policy", critic="discrete_q_network").  What differs from
    the continuous class above:

      networks      the actor (discrete_policy) and the two critics (discrete_q_network) have one shape, head -> l -> A outputs; each lives in
                    an ops.RainbowNet of its own (kind "pi" / "q": raw logits, Q rows) with its buckets, backward and plain Adam.  Constructed in
                    the reference's order (actor, critic 1 and its target, critic 2 and its target: sac.py:75-95), so one torch.manual_seed
                    gives its weights.  The actor's target bucket stays idle.
      learn()       gather into ONE [s; s'] block -> the actor over both halves (it does not step between its two uses) -> each critic's
                    online(s) and target(s') -> jh_sacd_critic_loss (the expectation of the target Q under pi', the categorical entropy, both
                    MSE losses and head gradients) -> both critics' backward and Adam -> both critics' online(s) AGAIN (sac.py:235-237 reads the
                    stepped critics) -> jh_sacd_actor_loss (the actor's loss and its gradient to the raw logits, alpha_loss, and the
                    temperature's refresh and Adam step on the device) -> the actor's backward and Adam.  One hipGraph after a warm eager call.
      temperature   ops.sacd_temperature: the MPO family's multiplier block (one Adam step for every learned scalar, csrc/jh_mult.h) with a
                    hyper block of its own for alpha_lr and the step count; learn k uses exp(log_alpha) after k - 1 steps, as the continuous agent.
      process()     sac.py:281-310: the lr decay reaches the three networks' optimizers, never alpha's; every target_update_period steps the
                    targets are overwritten by their online critics.
      act()         torch.multinomial on the device in training, argmax in evaluation, on the softmax of the native actor's logits.
                    manager.DeviceCollector on ops.DeviceCartPole runs the same rule inside one kernel for T timesteps of W envs
                    (csrc/jh_devroll_disc.hip), on the collectors' counter-based stream instead of torch's.

    Departures on purpose: log pi is a log-softmax, clamped as Categorical clamps its probabilities (the same entropy wherever float32 pi is a
    normal number, finite beyond); load() as the continuous class (critic 2 from "critic2", targets equal their online critics, the alpha in
    use follows the loaded log_alpha)."""

    action_type = "discrete"
    _RESUME_ATTRS = SAC._RESUME_ATTRS + ("_adam_steps_critic2",)
    NETS = (("actor", "actor_optimizer"), ("critic1", "critic_optimizer1"), ("critic2", "critic_optimizer2"))
    ACTOR_VIEW = RESULT_KEYS = None

    def _continuous_only(self, *args, **kwargs):
        raise NotImplementedError("the continuous SAC's one-object path (ops.SACNet): the discrete agent learns through learn() over its three RainbowNets and "
                                  "overwrites its targets (update_target_hard)")

    update_target_soft = _learn = _learn_stats = _critic_names = _make_net = _continuous_only

    def __init__(self, state_size, action_size, hidden_size=512, actor="continuous_policy", critic="continuous_q_network", head="mlp",
                 optim_config={"actor": "adam", "critic": "adam", "alpha": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3, "alpha_lr": 3e-4}, use_dynamic_alpha=False,
                 gamma=0.99, tau=5e-3, buffer_size=50000, batch_size=64, start_train_step=2000, static_log_alpha=-2.0, target_update_period=10000, run_step=1e6,
                 lr_decay=True, device=None, use_graph=True, **kwargs):
        is_int = lambda v: isinstance(v, (int, np.integer))
        ok_opt = (isinstance(optim_config, dict) and set(optim_config) <= {o + s for o in self.OPTIMIZERS for s in ("", "_lr")}
                  and all(str(optim_config.get(o, "adam")).lower() == "adam" for o in self.OPTIMIZERS))
        ok = (actor == "discrete_policy" and critic == "discrete_q_network" and head == "mlp" and np.isscalar(state_size) and is_int(action_size)
              and 2 <= action_size <= ops.SACD_MAX_ACTIONS and is_int(batch_size) and 1 <= batch_size <= ops.SACD_MAX_ROWS and is_int(hidden_size)
              and hidden_size % 4 == 0 and ok_opt and kwargs.get("grad_sync") is None)
        # process() learns only while memory.size > batch_size (strict, sac.py:289): a replay that cannot hold more than one batch would never learn, and
        # the discrete pair at such a configuration was refused before this class existed (tests/test_sac_gpu.py): it stays refused
        # Without a GPU the pair keeps its earlier answer too, the eligibility text before any GPU use (tests/test_sac_cpu.py), not _require_gpu's RuntimeError
        dev = torch.device(device) if device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if not ok or not buffer_size > batch_size or dev.type != "cuda":
            raise ValueError(f"{SAC_ELIGIBLE}; got actor={actor!r}, critic={critic!r}, head={head!r}, state_size={state_size!r}, action_size={action_size!r}, "
                             f"hidden_size={hidden_size!r}, batch_size={batch_size!r}, buffer_size={buffer_size!r}, optim_config={optim_config!r}, device={str(dev)!r}")
        self.device = self._require_gpu(device)
        self.use_graph, self.grad_sync = use_graph, None
        self.head, self.state_size, self.action_size, self.hidden_size, self.batch_size = head, int(state_size), int(action_size), int(hidden_size), int(batch_size)
        S, A, H, B = self.state_size, self.action_size, self.hidden_size, self.batch_size
        # sac.py:75-95: five constructions in this order; the targets' own initialisations are drawn and then overwritten
        inits = [Network(name, state_size, action_size, D_hidden=hidden_size, head=head) for name in (actor, critic, critic, critic, critic)]
        self._nets = {"actor": ops.RainbowNet(S, A, 1, H, head, B, self.device, kind="pi"), "critic1": ops.RainbowNet(S, A, 1, H, head, B, self.device, kind="q"),
                      "critic2": ops.RainbowNet(S, A, 1, H, head, B, self.device, kind="q")}
        for name, init in (("actor", inits[0]), ("critic1", inits[1]), ("critic2", inits[3])):
            self._nets[name].import_state(init.state_dict())
            self._nets[name].sync_target()
        self._net = self._nets["actor"]  # the marker of a native agent
        self.actor = self.network = NativeNet(self._nets["actor"], 0)  # BaseAgent.sync_in / sync_out carry the actor only (sac.py:345-355)
        for name in ("critic1", "critic2"):
            setattr(self, name, NativeNet(self._nets[name], 0))
            setattr(self, "target_" + name, NativeNet(self._nets[name], 1))
        self._lr0 = {"actor": float(optim_config.get("actor_lr", self.ACTOR_LR)), "critic": float(optim_config.get("critic_lr", 1e-3))}
        self._lr_now = dict(self._lr0)
        self._adam_steps_actor = self._adam_steps_critic = self._adam_steps_critic2 = 0
        for name, net in self._nets.items():
            net.set_hyper(self._lr0["actor" if name == "actor" else "critic"], 0.9, 0.999, 1e-8, 0)
        self.use_dynamic_alpha = bool(use_dynamic_alpha)
        self.alpha_lr = float(optim_config.get("alpha_lr", 3e-4))  # never decayed (sac.py:292-300)
        self.target_entropy = -np.log(1 / self.action_size) * 0.98
        self._set_temperature(0.0 if self.use_dynamic_alpha else static_log_alpha)
        self.gamma, self.tau = gamma, tau
        self.buffer_size = buffer_size
        self.memory = ReplayBuffer(buffer_size, device=self.device)
        self.memory.defer_rows = 16  # per-step stores coalesce into one ring append before the next learn()
        self.start_train_step, self.run_step, self.lr_decay = start_train_step, run_step, lr_decay
        self.num_learn, self.time_t = 0, 0
        self.target_update_stamp, self.target_update_period = 0, target_update_period
        self._stats = torch.zeros(len(ops.SACD_STATS), dtype=torch.float32, device=self.device)
        self._static, self._learn_graphs = None, ops.LearnGraphs("SACDiscrete.learn()")

    # ------------------------------------------------------------------------------------------ the temperature
    def _set_temperature(self, log_alpha, alpha=None, lr=None, beta1=0.9, beta2=0.999, eps=1e-8, step=0, m=0.0, v=0.0):
        """New device blocks (the captured graph holds the old ones' addresses: dropped)."""
        self._temp = ops.sacd_temperature(log_alpha, self.target_entropy, alpha, m, v, has_state=step > 0, device=self.device)
        self._temp_hyper = ops.vmpo_hyper(self.alpha_lr if lr is None else lr, beta1, beta2, eps, step, device=self.device)
        if getattr(self, "_learn_graphs", None) is not None:
            self.reset_graphs()

    def temperature(self):
        """-> {"log_alpha", "alpha" (in use), "m", "v", "lr", "beta1", "beta2", "eps", "step"} as Python numbers (synchronises)."""
        blk, h = ops.vmpo_block_read(self._temp), self._temp_hyper.cpu().numpy()
        b1, b2 = (float(x) for x in h[10:14].view(np.float64))
        return {"log_alpha": blk["eta"]["value"], "alpha": blk["alpha_mu"]["value"], "m": blk["eta"]["m"], "v": blk["eta"]["v"], "lr": float(h[0]), "beta1": b1,
                "beta2": b2, "eps": float(h[3]), "step": int(h[4])}

    log_alpha = property(lambda self: self.temperature()["log_alpha"])
    alpha = property(lambda self: self.temperature()["alpha"], doc="The alpha the next learn() forms its losses with.")

    # ------------------------------------------------------------------------------------------ acting
    @torch.no_grad()
    def act(self, state, training=True):
        """sac.py:151-159."""
        self.actor.train(training)
        pi = torch.softmax(self.actor(self.as_tensor(state)), dim=-1)
        action = torch.multinomial(pi, 1) if training else torch.argmax(pi, dim=-1, keepdim=True)
        return {"action": action.cpu().numpy()}

    # ------------------------------------------------------------------------------------------ learning
    def _alloc_static(self):
        """Fixed-address buffers of one learn(): the sampled rows, the gathered batch as one [s; s'] block, the networks' outputs, the head gradients."""
        B, A = self.batch_size, self.action_size
        idx = torch.zeros(B, dtype=torch.int64, device=self.device)
        probe = self.memory.gather(idx, as_float=True)
        if int(probe["state"].numel()) != B * self.state_size or int(probe["action"].numel()) != B:
            raise ValueError(f"SAC.learn(): stored rows are state {tuple(probe['state'].shape[1:])} / action {tuple(probe['action'].shape[1:])}, "
                             f"expected ({self.state_size},) / (1,): a discrete action is stored as its index")
        x_all = torch.empty(2 * B, self.state_size, dtype=torch.float32, device=self.device)
        tr = dict(probe)
        tr["state"], tr["next_state"] = x_all[:B], x_all[B:]
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)
        return dict(idx=idx, tr=tr, store=self.memory._store, x_all=x_all, la=f(3, B, A, 1), lq=(f(3, B, A, 1), f(3, B, A, 1)), q_pi=f(2, B, A, 1),
                    g_q=(f(B, A), f(B, A)), g_la=f(B, A), work=ops.sacd_workspace(self.device))

    def _draw(self, st):
        """The host side of one learn(), in front of the (replayed) body: the sampled rows."""
        from ..buffer.base import h2d_small

        st["idx"].copy_(h2d_small(self.memory.sample_indices(self.batch_size).astype(np.int64), self.device))

    def _learn_body(self, st):
        B, A = self.batch_size, self.action_size
        actor, critics = self._nets["actor"], (self._nets["critic1"], self._nets["critic2"])
        tr = self.memory.gather(st["idx"], as_float=True, out=st["tr"])
        la = actor.learn_forward(st["x_all"], B, None, st["la"])  # [0] online(s), [1] online(s'): one trunk pass over all 2B rows
        lq = [net.learn_forward(st["x_all"], B, None, out) for net, out in zip(critics, st["lq"])]  # [0] online(s), [2] target(s')
        g_q1, g_q2, _ = ops.sacd_critic_loss(la[1].view(B, A), lq[0][2].view(B, A), lq[1][2].view(B, A), lq[0][0].view(B, A), lq[1][0].view(B, A), tr["action"],
                                             tr["reward"], tr["done"], self.gamma, self._temp, stats=self._stats, work=st["work"], out=st["g_q"])
        for net, g in zip(critics, (g_q1, g_q2)):
            net.backward(g)
            net.optim_step("adam", None)
        q_pi = [net.forward(st["x_all"][:B], 0, None, out=st["q_pi"][i]) for i, net in enumerate(critics)]  # the stepped critics (sac.py:236-237)
        g_la, _ = ops.sacd_actor_loss(la[0].view(B, A), q_pi[0].view(B, A), q_pi[1].view(B, A), self._temp, self._temp_hyper, self.use_dynamic_alpha,
                                      stats=self._stats, work=st["work"], out=st["g_la"])
        actor.backward(g_la)
        actor.optim_step("adam", None)

    def learn(self):
        """sac.py:171-269.  Moves no target."""
        if self._static is None or self._static["store"] is not self.memory._store:
            self._static = self._alloc_static()
            self.reset_graphs()
        st = self._static
        self.memory.flush()
        self._draw(st)
        self._learn_graphs.run("learn", lambda: self._learn_body(st), self.use_graph)
        self.num_learn += 1
        self._adam_steps_actor += 1
        self._adam_steps_critic += 1
        self._adam_steps_critic2 += 1
        s = self._read_stats(self._stats)[0]
        self.result = {k: float(s[j]) for j, k in enumerate(ops.SACD_STATS)}
        return self.result

    def learning_rate_decay(self, step, optimizers=None, mode="cosine"):
        """base.py:93-111 on the actor's and the two critics' optimizers (sac.py:292-300); alpha's lr stays."""
        w = float(self._lr_weight(step, mode))
        for name, net in self._nets.items():
            which = "actor" if name == "actor" else "critic"
            self._lr_now[which] = self._lr0[which] * w
            net.set_lr(self._lr_now[which])  # a device scalar: the captured graph reads it

    def update_target_hard(self):
        self._nets["critic1"].sync_target()
        self._nets["critic2"].sync_target()

    def process(self, transitions, step):
        """sac.py:281-310: learns when memory.size > batch_size (strict); once learning has begun, the targets are overwritten whenever
        target_update_period steps have passed since the last time."""
        result = {}
        self._store(transitions)
        self.target_update_stamp += step - self.time_t
        self.time_t = step
        if self.memory.size > self.batch_size and step >= self.start_train_step:
            result = self.learn()
            if self.lr_decay:
                self.learning_rate_decay(step)
        if self.num_learn > 0 and self.target_update_stamp >= self.target_update_period:
            self.update_target_hard()
            self.target_update_stamp = 0
        return result

    # ------------------------------------------------------------------------------------------ checkpoints
    def _steps_of(self, name):
        return {"actor": self._adam_steps_actor, "critic1": self._adam_steps_critic, "critic2": self._adam_steps_critic2}[name]

    def _ckpt(self):
        """The reference's keys in its order (sac.py:312-326)."""
        shadows = {name: shadow_of(self._nets[name], {"name": "adam"}, self._lr_now["actor" if name == "actor" else "critic"]) for name, _ in self.NETS}
        for name, (opt, params, _) in shadows.items():
            if self._steps_of(name) > 0:
                optim_state.fill(opt, params, self._steps_of(name), *moments_of(self._nets[name]))
        sd = {name: self._nets[name].export_state() for name, _ in self.NETS}
        out = {"actor": sd["actor"], "actor_optimizer": shadows["actor"][0].state_dict(), "critic1": sd["critic1"], "critic2": sd["critic2"],
               "critic_optimizer1": shadows["critic1"][0].state_dict(), "critic_optimizer2": shadows["critic2"][0].state_dict()}
        if self.use_dynamic_alpha:
            t = self.temperature()
            opt, params = optim_state.shadow({"name": "adam", "betas": (t["beta1"], t["beta2"]), "eps": t["eps"]}, [self._one(t["log_alpha"])], t["lr"])
            if t["step"] > 0:
                optim_state.fill(opt, params, t["step"], [self._one(t["m"])], [self._one(t["v"])])
            out["log_alpha"], out["alpha_optimizer"] = params[0].detach(), opt.state_dict()
        return out

    def _load_ckpt(self, ckpt):
        for name, okey in self.NETS:
            net = self._nets[name]
            net.import_state(ckpt[name])
            net.sync_target()
            opt, params, keys = shadow_of(net, {"name": "adam"}, 0.0)
            opt.load_state_dict(ckpt[okey])
            steps = load_moments(net, keys, opt, params)
            lr, beta1, beta2, eps, _ = optim_state.hyper(opt.param_groups[0])
            net.set_hyper(lr, beta1, beta2, eps, steps)
            self._lr_now["actor" if name == "actor" else "critic"] = lr
            setattr(self, {"actor": "_adam_steps_actor", "critic1": "_adam_steps_critic", "critic2": "_adam_steps_critic2"}[name], steps)

    def load(self, path):
        """The reference's ckpt with the continuous class's departures: critic 2 from "critic2", both targets equal their loaded online critics,
        and the alpha in use becomes exp(loaded log_alpha) with the alpha optimizer's state restored."""
        print(f"...Load model from {path}...")
        ckpt = torch.load(os.path.join(path, "ckpt"), map_location=self.device, weights_only=False)
        self._load_ckpt(ckpt)
        if self.use_dynamic_alpha and "log_alpha" in ckpt:
            la = float(torch.as_tensor(ckpt["log_alpha"]).reshape(-1)[0])
            opt, params = optim_state.shadow({"name": "adam"}, [self._one(la)], self.alpha_lr)
            opt.load_state_dict(ckpt["alpha_optimizer"])
            steps, m, v = optim_state.read(opt, params)
            lr, beta1, beta2, eps, _ = optim_state.hyper(opt.param_groups[0])
            self._set_temperature(la, None, lr, beta1, beta2, eps, steps, float(optim_state.dense(m, params)[0]), float(optim_state.dense(v, params)[0]))

    def save_full(self, path, version=None):
        """BaseAgent's format version 2 only.  Beside the replay buffer, the counters (the target update stamp among them) and the generators it
        carries the two target critics and the whole temperature (block and hyper block, exact): a resumed run continues bit for bit."""
        if version not in (None, 2):
            raise ValueError(f"SAC.save_full writes resume format version 2 only, got version={version!r}")
        BaseAgent.save_full(self, path, version)
        d = os.path.join(path, "resume")
        torch.save({name: self._nets[name].export_state(self._nets[name].target) for name in ("critic1", "critic2")}, os.path.join(d, "targets.pt"))

    def load_full(self, path):
        BaseAgent.load_full(self, path)
        f = os.path.join(path, "resume", "targets.pt")
        if os.path.exists(f):
            for name, sd in torch.load(f, map_location=self.device, weights_only=False).items():
                self._nets[name].import_state(sd, self._nets[name].target)

    def _resume_extra_attrs(self):
        t = self.temperature()
        return {"sacd_block": ops.vmpo_block_hex(self._temp), "sacd_hyper": [float(t[k]).hex() for k in ("lr", "beta1", "beta2", "eps")] + [t["step"]]}

    def _resume_load_extra_attrs(self, d):
        if "sacd_block" in d:  # in place: the captured graph keeps reading these addresses
            ops.vmpo_block_from_hex(self._temp, d["sacd_block"])
            lr, beta1, beta2, eps = (float.fromhex(x) for x in d["sacd_hyper"][:4])
            self._temp_hyper.copy_(ops.vmpo_hyper(lr, beta1, beta2, eps, d["sacd_hyper"][4], device=self.device))
