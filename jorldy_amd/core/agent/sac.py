import os

import numpy as np
import torch

from ... import ops
from . import optim_state
from .base import BaseAgent
from .td3 import ActorCriticView, DeterministicActorCritic

SAC_ELIGIBLE = ("SAC runs on libjorldy_hip only: actor 'continuous_policy', critic 'continuous_q_network', head 'mlp' with a scalar state_size, "
                "hidden_size % 4 == 0, action_size >= 1, optim_config {'actor': 'adam', 'critic': 'adam', 'alpha': 'adam', actor_lr, critic_lr, alpha_lr} "
                "(config.sac x mujoco / pendulum / cartpole / hopper_mlagent and their shapes); the discrete SAC (discrete_policy / discrete_q_network) "
                "and the cnn head are not on the native engine")


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
