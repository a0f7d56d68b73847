import os

import numpy as np
import torch

from ... import ops
from ..network import Network
from ..optimizer import Optimizer
from .ppo import MAX_HEAD_OUTPUTS, PPO, export_views, import_views

MAX_MINIBATCH = ops.ICMNet.MAX_BATCH  # jh_icmnet_*: rows of one call
ICM_ELIGIBLE = ("ICM-PPO runs on libjorldy_hip only: network in {discrete_policy_value, continuous_policy_value}, head='mlp', int state_size, "
                "hidden_size % 16 == 0, optim_config name 'adam' without weight_decay / amsgrad, action_size + 1 (discrete) or 2 * action_size + 1 "
                f"(continuous) <= {MAX_HEAD_OUTPUTS} head outputs, icm_network='icm_mlp', lamb == 1.0 (the scale sits inside PPO's loss in front of the clip) "
                f"and batch_size <= {MAX_MINIBATCH} (config.icm_ppo.cartpole, .mountaincar, .pong_mlagent); the cnn head, icm_cnn / icm_multi, the "
                "*_separate_value networks, data-parallel learners and the native collector's acting-time capture are not available for this agent")
_BN = ("bn1", "bn2", "bn1_next")


class ICM_PPO(PPO):
    """core/agent/icm_ppo.py:14-238 on PPO's native machinery (the rollout store, ops.PPONet, act() and process(), the epoch shuffles, the
    statistics in device-mapped memory, the whole learn() as one hipGraph) plus the curiosity module as ops.ICMNet.  What differs from PPO:

      pre-pass      after the gather: icm.update_rms_obs(next_state), then the no-grad pass r_i = icm(s, a, s', update_ri=True) over the whole
                    rollout and reward <- extrinsic_coeff * reward + intrinsic_coeff * r_i in place (icm_ppo.py:96-102); PPO's pre-pass follows
                    on the mixed reward, unchanged.
      minibatches   PPO's updates as they are, whichever update path is selected; then the ICM's n_upd updates over the same index slices
                    (icm_ppo.py:177, 185, 194-199).  The two parameter sets are disjoint, so enqueuing all ICM updates behind all PPO updates
                    gives the reference's numbers.
      optimizers    two: learning_rate_decay reaches self.optimizer only (base.py:103-104); the ICM's Adam keeps its initial learning rate.

    self.icm is the parameter container (network.ICM_MLP): its 18 trainable Parameters are views of the native bucket; its first seven
    (rms_obs, rms_ri, rff) and the batch norms' buffers mirror the device statistics block when save() / sync asks for them.
    save() / load() are the reference's {"network", "icm", "optimizer", "icm_optimizer"}."""

    def __init__(self, state_size, action_size, hidden_size=512, optim_config={"name": "adam"}, icm_network="icm_mlp", beta=0.2, lamb=1.0, eta=0.01,
                 extrinsic_coeff=1.0, intrinsic_coeff=1.0, obs_normalize=True, ri_normalize=True, batch_norm=True, **kwargs):
        network, head = kwargs.get("network", "discrete_policy_value"), kwargs.get("head", "mlp")
        batch_size = kwargs.get("batch_size", 32)
        cont = network == "continuous_policy_value"
        ok = (head == "mlp" and isinstance(state_size, (int, np.integer)) and network in ("discrete_policy_value", "continuous_policy_value")
              and isinstance(hidden_size, (int, np.integer)) and hidden_size % 16 == 0 and isinstance(optim_config, dict)
              and str(optim_config.get("name", "adam")).lower() == "adam" and not optim_config.get("amsgrad", False) and not optim_config.get("weight_decay", 0)
              and isinstance(action_size, (int, np.integer)) and action_size >= 1 and (2 * action_size + 1 if cont else action_size + 1) <= MAX_HEAD_OUTPUTS
              and str(icm_network).lower() == "icm_mlp" and float(lamb) == 1.0 and 1 <= batch_size <= MAX_MINIBATCH)
        if not ok:
            raise ValueError(f"{ICM_ELIGIBLE}; got network={network!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size!r}, "
                             f"optim_config={optim_config!r}, action_size={action_size!r}, icm_network={icm_network!r}, lamb={lamb!r}, batch_size={batch_size!r}")
        super().__init__(state_size=state_size, action_size=action_size, hidden_size=hidden_size, optim_config=optim_config, **kwargs)
        self.obs_normalize, self.ri_normalize, self.batch_norm = obs_normalize, ri_normalize, batch_norm
        self.icm = Network(icm_network, state_size, action_size, self.num_workers, self.gamma, eta, self.action_type, ri_normalize, obs_normalize, batch_norm,
                           D_hidden=hidden_size).to(self.device)
        self.icm_optimizer = Optimizer(**optim_config, params=self.icm.parameters())
        self.beta, self.lamb, self.eta = beta, lamb, eta
        self.extrinsic_coeff, self.intrinsic_coeff = extrinsic_coeff, intrinsic_coeff
        self._icm_steps = 0    # Adam steps the ICM's optimizer has taken
        self._icm_batches = 0  # num_batches_tracked of every batch norm: 1 + n_upd per learn()
        self._icm_net = None
        self._init_icm(max(int(batch_size), min(int(self.n_step) * int(self.num_workers), MAX_MINIBATCH)))

    # ---------------------------------------------------------------------------------- the native module
    def _trainable(self):
        return [p for p in self.icm.parameters() if p.requires_grad]

    def _init_icm(self, max_batch):
        """(Re)build the native object for calls of up to max_batch rows.  The buckets stay (the nn.Parameters are views of them); the
        statistics block and the optimizer's settings are carried over."""
        old = self._icm_net
        net = ops.ICMNet(self._net.S, self._net.H, self._net.A, self._net.cont, self.num_workers, max_batch, self.device, eta=self.eta, gamma=self.gamma,
                         obs_normalize=self.obs_normalize, ri_normalize=self.ri_normalize, batch_norm=self.batch_norm,
                         buckets=None if old is None else (old.params, old.grads, old.m, old.v))
        params = self._trainable()
        assert [tuple(p.shape) for p in params] == [tuple(v.shape) for _, v in net._pairs(net.params)], "state_dict layout mismatch with libjorldy_hip"
        if old is None:
            with torch.no_grad():
                for p, (_, v), (_, g) in zip(params, net._pairs(net.params), net._pairs(net.grads)):
                    v.copy_(p)
                    p.data = v  # nn.Parameters become views of the bucket
                    p.grad = g
            self._icm_views = [(p, m, v) for p, (_, m), (_, v) in zip(params, net._pairs(net.m), net._pairs(net.v))]
        else:
            net.set_stats(old.stats())
        d = self.icm_optimizer.defaults
        net.set_hyper(self.icm_optimizer.param_groups[0]["lr"], d["betas"][0], d["betas"][1], d["eps"], step=self._icm_steps)
        torch.cuda.synchronize()
        self._icm_net = net
        if old is not None:
            self._static = None
            self.reset_graphs()

    # ---------------------------------------------------------------------------------- what this agent does not take part in
    def _capture_targets(self, M):
        raise NotImplementedError("ICM-PPO: the native collector's acting-time capture is PPO's (the pre-pass needs the intrinsic reward before the values)")

    def process_begin(self, step):
        raise NotImplementedError("ICM-PPO: the native collector's begin / loop form of process() is PPO's; use process()")

    def process_end(self):
        raise NotImplementedError("ICM-PPO: the native collector's begin / loop form of process() is PPO's; use process()")

    def early_ready(self):
        return False

    # ---------------------------------------------------------------------------------- learn
    def learn(self):
        if self.grad_sync is not None:
            raise NotImplementedError("ICM-PPO: data-parallel learners (grad_sync) are not available: the module's gradients and batch statistics would need their own reductions")
        M, B = self.memory.size, self.batch_size
        if M < 2:
            raise ValueError(f"ICM-PPO: a rollout of {M} row(s): the observation moments need more than one row (x.std of one row is NaN, utils.py:26-29)")
        if M % self.num_workers != 0:
            raise ValueError(f"ICM-PPO: a rollout of {M} rows does not divide among num_workers={self.num_workers} (r_i.view(num_workers, -1), icm.py:146)")
        if self.batch_norm and M % B == 1:
            raise ValueError(f"ICM-PPO: a rollout of {M} rows leaves a last minibatch of ONE row at batch_size {B}: a training-mode batch norm raises "
                             "'Expected more than 1 value per channel' there (icm.py:20-25)")
        if M > MAX_MINIBATCH:
            raise ValueError(f"ICM-PPO: a rollout of {M} rows exceeds the {MAX_MINIBATCH} rows the module's no-grad pass takes in one call (its batch norms "
                             "use the statistics of the whole rollout)")
        if M > self._icm_net.maxB:
            self._init_icm(M)
        result = self._learn_native()
        n_upd = self._static["n_upd"]
        self._icm_steps += n_upd
        self._icm_batches += 1 + n_upd
        return result

    def _alloc_static(self, M):
        st = super()._alloc_static(M)
        n_upd = st["n_upd"]
        # the ICM's rows {l_f, l_i, 0, mark} and, in row n_upd, mean(r_i) of the pre-pass: a mapped buffer of their own
        st["icm_pin"] = self._mapped_stats(n_upd + 1, 4)
        st["icm_stats"] = st["icm_pin"].dev
        return st

    def _enqueue_pre(self, st, captured=False):
        """icm_ppo.py:96-112: the gather, the observation moments, the intrinsic reward mixed into the reward column, PPO's pre-pass."""
        assert not captured
        tr, icm = st["tr"], self._icm_net
        self._enqueue_gather(st)
        icm.obs_update(tr["next_state"])
        icm.reward(tr["state"], tr["next_state"], tr["action"], tr["reward"], self.extrinsic_coeff, self.intrinsic_coeff, ri_mean=st["icm_stats"][st["n_upd"]])
        self._enqueue_pre_pass(st)

    def _enqueue_main(self, st):
        """icm_ppo.py:136-199: PPO's minibatch updates, then the module's over the same index slices."""
        super()._enqueue_main(st)
        icm, tr, M, B = self._icm_net, st["tr"], st["M"], self.batch_size
        k = 0
        for e in range(self.n_epoch):
            for offset in range(0, M, B):
                b = min(B, M - offset)
                icm.update(tr["state"], tr["next_state"], tr["action"], st["idx"][e * M + offset : e * M + offset + b], self.beta, self.clip_grad_norm,
                           stats=st["icm_stats"][k])
                k += 1

    def _stat_marks(self, n_upd):
        return {**super()._stat_marks(n_upd), "icm_pin": ((n_upd - 1) * 4 + 3,)}  # jh_icm.hip writes [3] last, behind a system-scope fence

    def _result(self, s, n_upd):
        a = self._static["icm_pin"].np.astype(np.float64)
        result = super()._result(s, n_upd)
        result.update({"r_i": float(a[n_upd, 0]), "l_f": float(a[n_upd - 1, 0]), "l_i": float(a[n_upd - 1, 1])})  # the LAST minibatch's losses (icm_ppo.py:215-216)
        return result

    # ---------------------------------------------------------------------------------- checkpoint
    def _sync_icm_out(self):
        """Device statistics block -> the container's buffer-like Parameters and the batch norms' buffers."""
        blk = self._icm_net.stats()
        with torch.no_grad():
            for k in ("rms_obs.mean", "rms_obs.var", "rms_obs.count", "rms_ri.mean", "rms_ri.var", "rms_ri.count", "rff.rewems"):
                mod, name = k.split(".")
                getattr(getattr(self.icm, mod), name).copy_(torch.from_numpy(blk[k]))
            if self.batch_norm:
                for bn in _BN:
                    m = getattr(self.icm, bn)
                    m.running_mean.copy_(torch.from_numpy(blk[bn + ".running_mean"]))
                    m.running_var.copy_(torch.from_numpy(blk[bn + ".running_var"]))
                    m.num_batches_tracked.fill_(self._icm_batches)

    def _sync_icm_in(self):
        """The container (after load_state_dict) -> the device statistics block and the batch counter."""
        sd = self.icm.state_dict()
        self._icm_net.set_stats({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
        if self.batch_norm:
            self._icm_batches = int(self.icm.bn1.num_batches_tracked)

    def _export_optim_state(self):
        super()._export_optim_state()
        export_views(self.icm_optimizer, self._icm_views, self._icm_steps)  # the first seven parameters never get a gradient: no views, no state

    def _import_optim_state(self):
        super()._import_optim_state()
        if self._icm_net is None:
            return
        self._icm_steps = steps = import_views(self.icm_optimizer, self._icm_views)
        d = self.icm_optimizer.defaults
        self._icm_net.set_hyper(self.icm_optimizer.param_groups[0]["lr"], d["betas"][0], d["betas"][1], d["eps"], step=steps)

    def _resume_extra_attrs(self):
        d = super()._resume_extra_attrs()
        d["icm_steps"], d["icm_batches"] = int(self._icm_steps), int(self._icm_batches)
        return d

    def _resume_load_extra_attrs(self, d):
        super()._resume_load_extra_attrs(d)
        self._icm_steps, self._icm_batches = int(d.get("icm_steps", self._icm_steps)), int(d.get("icm_batches", self._icm_batches))

    def save(self, path):
        print(f"...Save model to {path}...")
        self._export_optim_state()
        self._sync_icm_out()
        torch.save({"network": self.network.state_dict(), "icm": self.icm.state_dict(), "optimizer": self.optimizer.state_dict(),
                    "icm_optimizer": self.icm_optimizer.state_dict()}, os.path.join(path, "ckpt"))

    def load(self, path):
        print(f"...Load model from {path}...")
        checkpoint = torch.load(os.path.join(path, "ckpt"), map_location=self.device, weights_only=False)
        self.network.load_state_dict(checkpoint["network"])
        self.icm.load_state_dict(checkpoint["icm"])
        self.optimizer.load_state_dict(checkpoint["optimizer"])
        self.icm_optimizer.load_state_dict(checkpoint["icm_optimizer"])
        torch.cuda.current_stream().synchronize()
        self._sync_icm_in()
        self._import_optim_state()
