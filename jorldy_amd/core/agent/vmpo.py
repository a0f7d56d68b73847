import os

import numpy as np
import torch

from ... import ops
from ..optimizer import Optimizer
from . import optim_state
from .ppo import MAX_HEAD_OUTPUTS, PPO

MAX_MINIBATCH = 1024  # jh_vmpo_loss_*: one workgroup, one row per thread
VMPO_ELIGIBLE = ("V-MPO runs on libjorldy_hip only: network in {discrete_policy_value, continuous_policy_value}, head='mlp', int state_size, "
                 "hidden_size % 16 == 0, optim_config name 'adam' without weight_decay / amsgrad, action_size + 1 (discrete) or 2 * action_size + 1 "
                 f"(continuous) <= {MAX_HEAD_OUTPUTS} head outputs, and batch_size <= {MAX_MINIBATCH}: the top half of a minibatch is selected inside one "
                 "workgroup (config.vmpo.cartpole, config.vmpo.mujoco on all its envs); the cnn head, data-parallel learners and the native "
                 "collector's acting-time capture are not available for this agent")


class VMPO(PPO):
    """core/agent/vmpo.py:10-291 on PPO's native machinery: the rollout store, ops.PPONet with the nn.Parameters as views of its bucket, act()
    and process(), the epoch shuffles drawn by numpy's own algorithm, the statistics in device-mapped memory, the lr decay through set_lr,
    and the whole learn() as one hipGraph after a warm eager call.  What differs from PPO:

      pre-pass      one forward over [s; s'], GAE with per-row standardisation (jh_gae; its `ret` is NOT V-MPO's, which is taken after the
                    standardisation, vmpo.py:153: the loss kernel forms adv + value_old itself).  No log pi_old: the reference computes and never uses it.
                    The raw old heads of the whole rollout stay: they are the *_old of the KL terms.
      minibatch     net.forward(idx) -> jh_vmpo_loss_* (top half above the lower median, psi, the four losses, head gradients, AND the three
                    Lagrange multipliers' Adam steps and floors on the device) -> net.backward -> clip_grad_norm_ over the NETWORK's parameters only +
                    Adam (vmpo.py:246-252).  The same launches as PPO's separate-call update with this loss kernel in the loss's place; PPO's fused
                    four-launch update has no V-MPO form.
      multipliers   eta, alpha_mu, alpha_sigma live in a device block (ops.vmpo_block) stepped by the loss kernel with the network's own lr, betas,
                    eps and step count (ONE optimizer holds them all, vmpo.py:87-91; the cosine decay reaches them).  Minibatch k sees them after
                    k - 1 steps.  A discrete policy never gives alpha_sigma a gradient: torch's Adam skips it, and so does the kernel.

    A rollout whose last minibatch is ONE row (M % batch_size == 1) has an empty top half there: the reference's eta turns NaN for good;
    learn() raises instead.  save() / load() are the reference's {"network", "optimizer"} (reinforce.py:128-142): the multipliers' VALUES are not
    part of it (their Adam moments are); save_full / load_full carry the whole block."""

    def __init__(self, state_size, action_size, hidden_size=512, network="discrete_policy_value", head="mlp", optim_config={"name": "adam"}, gamma=0.99,
                 use_standardization=True, run_step=1e6, lr_decay=True, device=None, batch_size=32, n_step=128, n_epoch=1, _lambda=0.9, clip_grad_norm=1.0,
                 min_eta=1e-8, min_alpha_mu=1e-8, min_alpha_sigma=1e-8, eps_eta=0.02, eps_alpha_mu=0.1, eps_alpha_sigma=0.1, eta=1.0, alpha_mu=1.0,
                 alpha_sigma=1.0, num_workers=1, use_graph=True, seed=0, **kwargs):
        cont = network == "continuous_policy_value"
        ok = (head == "mlp" and isinstance(state_size, (int, np.integer)) and network in ("discrete_policy_value", "continuous_policy_value")
              and isinstance(hidden_size, (int, np.integer)) and hidden_size % 16 == 0 and isinstance(optim_config, dict)
              and str(optim_config.get("name", "adam")).lower() == "adam" and not optim_config.get("amsgrad", False) and not optim_config.get("weight_decay", 0)
              and isinstance(action_size, (int, np.integer)) and action_size >= 1 and (2 * action_size + 1 if cont else action_size + 1) <= MAX_HEAD_OUTPUTS
              and 1 <= batch_size <= MAX_MINIBATCH)
        if not ok:
            raise ValueError(f"{VMPO_ELIGIBLE}; got network={network!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size!r}, "
                             f"optim_config={optim_config!r}, action_size={action_size!r}, batch_size={batch_size!r}")
        super().__init__(state_size, action_size, hidden_size=hidden_size, network=network, head=head, optim_config=optim_config, gamma=gamma,
                         use_standardization=use_standardization, run_step=run_step, lr_decay=lr_decay, device=device, batch_size=batch_size, n_step=n_step,
                         n_epoch=n_epoch, _lambda=_lambda, epsilon_clip=0.0, vf_coef=1.0, ent_coef=0.0, clip_grad_norm=clip_grad_norm, num_workers=num_workers,
                         use_graph=use_graph, seed=seed)
        self.fused_update = False  # jh_pponet_ppo_update is PPO's loss
        self.min_eta, self.min_alpha_mu, self.min_alpha_sigma = min_eta, min_alpha_mu, min_alpha_sigma
        self.eps_eta, self.eps_alpha_mu, self.eps_alpha_sigma = eps_eta, eps_alpha_mu, eps_alpha_sigma
        self._mult = ops.vmpo_block(eta, alpha_mu, alpha_sigma, min_eta, min_alpha_mu, min_alpha_sigma, eps_eta, eps_alpha_mu, eps_alpha_sigma, device=self.device)
        # ONE optimizer over the network's parameters and the three scalars (vmpo.py:87-91): the checkpoint's "optimizer" has this shape
        self._mult_params = [torch.nn.Parameter(torch.tensor(float(v), device=self.device)) for v in self._mult[:3].tolist()]
        d = self.optimizer.defaults
        self.optimizer = Optimizer(**optim_config, params=list(self.network.parameters()) + self._mult_params)
        assert self.optimizer.defaults["lr"] == d["lr"] and self.optimizer.defaults["betas"] == d["betas"]

    # ---------------------------------------------------------------------------------- the multipliers
    def multipliers(self):
        """ops.vmpo_block_read of the device block (synchronises)."""
        return ops.vmpo_block_read(self._mult)

    eta = property(lambda self: self.multipliers()["eta"]["value"])
    alpha_mu = property(lambda self: self.multipliers()["alpha_mu"]["value"])
    alpha_sigma = property(lambda self: self.multipliers()["alpha_sigma"]["value"])

    # ---------------------------------------------------------------------------------- what this agent does not take part in
    def _capture_targets(self, M):
        raise NotImplementedError("V-MPO: the native collector's acting-time capture is PPO's (the pre-pass keeps the raw old heads of its own forward)")

    def process_begin(self, step):
        raise NotImplementedError("V-MPO: the native collector's begin / loop form of process() is PPO's; use process()")

    def process_end(self):
        raise NotImplementedError("V-MPO: the native collector's begin / loop form of process() is PPO's; use process()")

    def early_ready(self):
        return False

    # ---------------------------------------------------------------------------------- learn
    def learn(self):
        if self.grad_sync is not None:
            raise NotImplementedError("V-MPO: data-parallel learners (grad_sync) are not available: the multipliers' gradients would need their own reduction")
        M = self.memory.size
        if M % self.batch_size == 1:
            raise ValueError(f"V-MPO: a rollout of {M} rows leaves a last minibatch of ONE row at batch_size {self.batch_size}: nothing lies above its median, and the "
                             "reference's eta_loss = log(mean of an empty top half) is NaN there, which turns eta NaN for good (vmpo.py:174-196)")
        return self._learn_native()

    def _result(self, s, n_upd):
        return {"actor_loss": np.mean(s[:n_upd, 0]), "critic_loss": np.mean(s[:n_upd, 1]), "eta_loss": np.mean(s[:n_upd, 2]), "alpha_loss": np.mean(s[:n_upd, 3]),
                "eta": float(s[n_upd - 1, 4]), "alpha_mu": float(s[n_upd - 1, 5]), "alpha_sigma": float(s[n_upd - 1, 6])}

    def _stat_marks(self, n_upd):
        return {"stats_pin": ((n_upd - 1) * 8 + 7,)}  # jh_vmpo.hip writes [7] last, behind a system-scope fence

    def _enqueue_pre(self, st, captured=False):
        """vmpo.py:111-153 without log pi_old and without ret."""
        net, M = self._net, st["M"]
        tr = st["tr"]
        self.memory._store.gather(st["arange"], as_float=True, out={k: tr[k] for k in tr})
        if 2 * M <= min(net.max_rows, 8192):
            net.forward(st["x_all"], out=(st["h0_all"], st["h1_all"], st["v_all"]))
        else:
            net.forward(tr["next_state"], out=(st["nh0"], st["nh1"], st["next_value"]))
            net.forward(tr["state"], out=(st["h0"], st["h1"], st["value"]))
        ops.gae(tr["reward"], tr["done"], st["value"], st["next_value"], self.n_step, self.gamma, self._lambda, self.use_standardization, out=(st["adv"], st["ret"]))

    def _enqueue_main(self, st):
        """vmpo.py:156-257: forward, loss + multipliers, backward, clip + Adam per minibatch."""
        net, M, B = self._net, st["M"], self.batch_size
        tr, adv, hyper = st["tr"], st["adv"], net.hyper_ptr()
        k = 0
        for e in range(self.n_epoch):
            for offset in range(0, M, B):
                b = min(B, M - offset)
                idx = st["idx"][e * M + offset : e * M + offset + b]
                if net.cont:
                    mu, ls, vp = net.forward(tr["state"], idx=idx, out=(st["mb_h0"][:b], st["mb_h1"][:b], st["mb_v"][:b]))
                    g_mu, g_ls, g_v, _ = ops.vmpo_loss_continuous(mu, ls, vp, idx, tr["action"], adv, st["value"], st["h0"], st["h1"], self._mult, hyper, stats=st["stats"][k])
                    net.backward(tr["state"], idx, g_mu, g_ls, g_v)
                else:
                    z, vp = net.forward(tr["state"], idx=idx, out=(st["mb_h0"][:b], None, st["mb_v"][:b]))
                    g_z, g_v, _ = ops.vmpo_loss_discrete(z, vp, idx, tr["action"], adv, st["value"], st["h0"], self._mult, hyper, stats=st["stats"][k])
                    net.backward(tr["state"], idx, g_z, None, g_v)
                net.adam_step(self.clip_grad_norm)
                k += 1

    # ---------------------------------------------------------------------------------- checkpoint
    def _resume_extra_attrs(self):
        d = super()._resume_extra_attrs()
        d["vmpo_block"] = ops.vmpo_block_hex(self._mult)
        return d

    def _resume_load_extra_attrs(self, d):
        super()._resume_load_extra_attrs(d)
        if "vmpo_block" in d:
            ops.vmpo_block_from_hex(self._mult, d["vmpo_block"])

    def _export_optim_state(self):
        """The network's moments as PPO exports them; the multipliers that have taken a step carry theirs, the others (alpha_sigma of a discrete
        policy) have no entry, as in torch's own optimizer."""
        super()._export_optim_state()
        with torch.no_grad():
            for p, value in zip(self._mult_params, self._mult[:3].tolist()):
                p.fill_(value)
        optim_state.fill(self.optimizer, self._mult_params, self._adam_steps, *ops.vmpo_block_moments(self._mult))

    def _import_optim_state(self):
        """The loaded optimizer's moments of the multipliers go into the device block; their VALUES are not in the reference's checkpoint and stay
        what they are (on a freshly constructed agent: the constructor's)."""
        super()._import_optim_state()
        _, m, v = optim_state.read(self.optimizer, self._mult_params)
        ops.vmpo_block_set_moments(self._mult, m, v)
