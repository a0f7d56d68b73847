import os

import numpy as np
import torch

from ... import ops
from ..network import Network
from ..optimizer import Optimizer
from .native_net import NativeNet, load_moments, moments_of, shadow_of
from . import optim_state
from .ppo import export_views, import_views
from .ppo_cnn import PackedHeadsPPO

MAX_ROWS = ops.RNDNet.MAX_BATCH  # jh_rndnet_*: rows of one call
MAX_ACTIONS = {"discrete": 64, "continuous": 32}  # jh_rnd_ppo_loss_packed
_KINDS = {"discrete_policy_separate_value": "pv2", "continuous_policy_separate_value": "gauss2"}
RND_ELIGIBLE = ("RND-PPO runs on libjorldy_hip only: network in {discrete_policy_separate_value, continuous_policy_separate_value}, head='mlp', int state_size, "
                "hidden_size % 4 == 0, optim_config {'name': 'adam', lr, betas, eps}, 2 <= action_size <= 64 (discrete) or 1 <= action_size <= 32 (continuous), "
                f"rnd_network='rnd_mlp' and batch_size <= {MAX_ROWS} (config.rnd_ppo.cartpole, .mountaincar, .pong_mlagent, .mujoco); the cnn and multi heads, "
                "rnd_cnn / rnd_multi, the networks with one value head, other optimizers, data-parallel learners (grad_sync) and the native collector's "
                "acting-time capture are not available for this agent")
_BN = ("bn1_predict_mlp", "bn2_predict_mlp", "bn1_target_mlp", "bn2_target_mlp")
_BLOCK_KEYS = ("rms_obs.mean", "rms_obs.var", "rms_obs.count", "rms_ri.mean", "rms_ri.var", "rms_ri.count", "rff.rewems")


class SeparateValueNet(NativeNet):
    """`agent.network` of the policy-value nets with two value heads: state_dict in the reference's keys (head.l, l, pi | mu, log_std, v, v_i:
    policy_value.py:25-35, 60-70) over the library's flat bucket; calling it returns (pi, v) or (mu, std, v) like the reference module's
    forward, `get_v_i` the intrinsic value."""

    @torch.no_grad()
    def raw(self, x):
        net = self._net
        x = x.contiguous().to(torch.float32)
        outs = [net.forward(x[o : o + net.maxB], self._which, None) for o in range(0, x.shape[0], net.maxB)]
        return (outs[0] if len(outs) == 1 else torch.cat(outs, 0)).view(-1, net.A)

    def __call__(self, x):
        out, n = self.raw(x), self._net.n_actions
        if self._net.kind == "pv2":
            return torch.softmax(out[:, :n], dim=-1), out[:, n : n + 1].clone()
        return torch.clamp(out[:, :n], min=-5.0, max=5.0), torch.tanh(out[:, n : 2 * n]).exp(), out[:, 2 * n : 2 * n + 1].clone()

    def get_v_i(self, x):
        return self.raw(x)[:, -1:].clone()


class RND_PPO(PackedHeadsPPO):
    """core/agent/rnd_ppo.py:14-307 on the native engine.

      network       head -> l -> (pi | v | v_i) or (mu | log_std | v | v_i): ops.RainbowNet kind "pv2" / "gauss2", a q-network whose last layer stacks
                    the heads, as PPO on the CNN head runs its policy-value net (ppo_cnn.py); the reference's module draws the initial weights.
      module        ops.RNDNet (jh_rnd.hip): predictor and frozen target, the running moments, the reward filter.  self.rnd is the parameter
                    container (network.RND_MLP): its 16 weight tensors are views of the native bucket; its first seven Parameters (rms_obs,
                    rms_ri, rff) and the batch norms' buffers mirror the device statistics block when save() asks for them.
      pre-pass      gather; rnd.update_rms_obs(next_state); r_i = rnd(next_state, update_ri=True); the net over [s; s'] unpacked to
                    pi | v | v_i; log pi_old; two jh_gae calls with standardize off (the intrinsic one with gamma_i and, when non_episodic, a
                    zero done column; non_extrinsic: a zero reward column for the extrinsic one); jh_rnd_adv_mix           rnd_ppo.py:112-166
      minibatches   forward (kept) -> jh_rnd_ppo_loss_packed -> backward -> clip + Adam, then the module's update on the same index slice
                    (the parameter sets are disjoint)                                                                     rnd_ppo.py:172-266
      optimizers    two: learning_rate_decay reaches the policy's only (base.py:103-104); the module's Adam keeps its learning rate.
      act()         rnd_ppo.py:85-99, returns {"action"} only.

    All of learn() is one hipGraph (ops.LearnGraphs) with one statistics read-back.  save() / load() are the reference's {"network", "rnd",
    "optimizer", "rnd_optimizer"}.  Departure on purpose: log pi is a log-softmax of the logits where the reference takes the log of a
    renormalised softmax (as MPO's and REINFORCE's kernels)."""

    def __init__(self, state_size, action_size, hidden_size=512, optim_config={"name": "adam"}, rnd_network="rnd_mlp", gamma_i=0.99, extrinsic_coeff=2.0,
                 intrinsic_coeff=1.0, obs_normalize=True, ri_normalize=True, batch_norm=True, non_episodic=True, non_extrinsic=False,
                 network="discrete_policy_value", head="mlp", gamma=0.99, use_standardization=True, run_step=1e6, lr_decay=True, device=None, batch_size=32,
                 n_step=128, n_epoch=3, _lambda=0.95, epsilon_clip=0.1, vf_coef=1.0, ent_coef=0.01, clip_grad_norm=1.0, num_workers=1, backend=None,
                 use_graph=True, seed=0, forward_rows=1024, grad_sync=None, **kwargs):
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        kind = _KINDS.get(network) if isinstance(network, str) else None
        a_type = network.split("_")[0] if kind else None
        ok = (kind is not None and head == "mlp" and is_int(state_size) and state_size >= 1 and is_int(hidden_size) and hidden_size > 0 and hidden_size % 4 == 0
              and isinstance(optim_config, dict) and str(optim_config.get("name", "adam")).lower() == "adam" and set(optim_config) <= {"name", "lr", "betas", "eps"}
              and is_int(action_size) and (2 if a_type == "discrete" else 1) <= action_size <= MAX_ACTIONS[a_type] and str(rnd_network).lower() == "rnd_mlp"
              and is_int(batch_size) and 1 <= batch_size <= MAX_ROWS and grad_sync is None and backend in (None, "auto", "native"))
        if not ok:
            raise ValueError(f"{RND_ELIGIBLE}; got network={network!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size!r}, optim_config={optim_config!r}, "
                             f"action_size={action_size!r}, rnd_network={rnd_network!r}, batch_size={batch_size!r}, grad_sync={grad_sync!r}, backend={backend!r}")
        self.device = self._require_gpu(device)
        self.action_type = a_type
        self.state_size, self.action_size, self.hidden_size = int(state_size), int(action_size), int(hidden_size)
        self.gamma, self.use_standardization, self.run_step, self.lr_decay = gamma, use_standardization, run_step, lr_decay
        self.batch_size, self.n_step, self.n_epoch, self._lambda = batch_size, n_step, n_epoch, _lambda
        self.epsilon_clip, self.vf_coef, self.ent_coef, self.clip_grad_norm, self.num_workers = epsilon_clip, vf_coef, ent_coef, clip_grad_norm, num_workers
        self.rnd_network, self.gamma_i, self.extrinsic_coeff, self.intrinsic_coeff = rnd_network, gamma_i, extrinsic_coeff, intrinsic_coeff
        self.obs_normalize, self.ri_normalize, self.batch_norm = obs_normalize, ri_normalize, batch_norm
        self.non_episodic, self.non_extrinsic = non_episodic, non_extrinsic
        self.use_graph = use_graph
        self._init_packed("RND_PPO.learn()", seed)
        # the reference draws the policy's weights first, then the module's (rnd_ppo.py:52-82): one torch.manual_seed gives both
        torch_net = Network(network, self.state_size, self.action_size, D_hidden=self.hidden_size, head=head)
        self._net = ops.RainbowNet(self.state_size, self.action_size, 1, self.hidden_size, "mlp", max(int(batch_size), int(forward_rows)), self.device, kind=kind)
        self._net.import_state(torch_net.state_dict())
        self.network = SeparateValueNet(self._net, 0)
        self._init_optimizer(optim_config)
        self.rnd = Network(rnd_network, self.state_size, self.action_size, self.num_workers, gamma_i, ri_normalize, obs_normalize, batch_norm,
                           D_hidden=self.hidden_size).to(self.device)
        self.rnd_optimizer = Optimizer(**optim_config, params=self.rnd.parameters())
        self._rnd_steps = 0    # Adam steps the module's optimizer has taken
        self._rnd_batches = 0  # num_batches_tracked of every batch norm: 1 + n_upd per learn()
        self._rnd_net = None
        self._init_rnd(max(int(batch_size), min(int(self.n_step) * int(self.num_workers), MAX_ROWS)))

    # ---------------------------------------------------------------------------------- the native module
    def _init_rnd(self, max_batch):
        """(Re)build the native object for calls of up to max_batch rows.  The buckets stay (the nn.Parameters are views of them); the
        statistics block and the optimizer's settings are carried over."""
        old = self._rnd_net
        net = ops.RNDNet(self.state_size, self.hidden_size, self.num_workers, max_batch, self.device, gamma_i=self.gamma_i, obs_normalize=self.obs_normalize,
                         ri_normalize=self.ri_normalize, batch_norm=self.batch_norm, buckets=None if old is None else (old.params, old.grads, old.m, old.v))
        named = dict(self.rnd.named_parameters())
        pairs = net._pairs(net.params)
        assert [tuple(named[k].shape) for k, _ in pairs] == [tuple(v.shape) for _, v in pairs] and len(pairs) + len(_BLOCK_KEYS) == len(named), \
            "state_dict layout mismatch with libjorldy_hip"
        if old is None:
            with torch.no_grad():
                for (k, v), (_, g) in zip(pairs, net._pairs(net.grads)):
                    p = named[k]
                    v.copy_(p)
                    p.data = v  # nn.Parameters become views of the bucket
                    if p.requires_grad:
                        p.grad = g
            self._rnd_views = [(named[k], m, v) for (k, m), (_, v) in zip(net._pairs(net.m, True), net._pairs(net.v, True))]
        else:
            net.set_stats(old.stats())
        d = self.rnd_optimizer.defaults
        net.set_hyper(self.rnd_optimizer.param_groups[0]["lr"], d["betas"][0], d["betas"][1], d["eps"], step=self._rnd_steps)
        torch.cuda.synchronize()
        self._rnd_net = net
        if old is not None:
            self._static = None
            self.reset_graphs()

    # ---------------------------------------------------------------------------------- what this agent does not take part in
    def _capture_targets(self, M):
        raise NotImplementedError("RND-PPO: the native collector's acting-time capture is PPO's (the pre-pass needs the intrinsic reward and a second value head)")

    def process_begin(self, step):
        raise NotImplementedError("RND-PPO: the native collector's begin / loop form of process() is PPO's; use process()")

    def process_end(self):
        raise NotImplementedError("RND-PPO: the native collector's begin / loop form of process() is PPO's; use process()")

    # ---------------------------------------------------------------------------------- act
    @torch.no_grad()
    def act(self, state, training=True):
        """rnd_ppo.py:85-99."""
        if isinstance(state, list):
            raise NotImplementedError("RND-PPO: list-valued (multimodal) observations are outside the native policy-value net")
        self.network.train(training)
        if self.action_type == "continuous":
            mu, std, _ = self.network(self.as_tensor(state))
            z = torch.normal(mu, std) if training else mu
            action = torch.tanh(z)
        else:
            pi, _ = self.network(self.as_tensor(state))
            action = torch.multinomial(pi, 1) if training else torch.argmax(pi, dim=-1, keepdim=True)
        return {"action": action.cpu().numpy()}

    # ---------------------------------------------------------------------------------- learn
    def learn(self):
        if self.grad_sync is not None:
            raise NotImplementedError("RND-PPO: data-parallel learners (grad_sync) are not available: the module's gradients and batch statistics would need their own reductions")
        M, B = self.memory.size, self.batch_size
        if M < 2:
            raise ValueError(f"RND-PPO: a rollout of {M} row(s): the observation moments need more than one row (x.std of one row is NaN, utils.py:26-29)")
        if M % self.num_workers != 0:
            raise ValueError(f"RND-PPO: a rollout of {M} rows does not divide among num_workers={self.num_workers} (r_i.view(num_workers, -1), rnd.py:160)")
        if M % self.n_step != 0:
            raise ValueError(f"RND-PPO: a rollout of {M} rows does not divide into rows of n_step={self.n_step} (adv.view(-1, n_step), rnd_ppo.py:141)")
        if self.batch_norm and M % B == 1:
            raise ValueError(f"RND-PPO: a rollout of {M} rows leaves a last minibatch of ONE row at batch_size {B}: a training-mode batch norm raises "
                             "'Expected more than 1 value per channel' there (rnd.py:38-44)")
        if M > MAX_ROWS:
            raise ValueError(f"RND-PPO: a rollout of {M} rows exceeds the {MAX_ROWS} rows the module's no-grad pass takes in one call (its batch norms "
                             "use the statistics of the whole rollout)")
        if M > self._rnd_net.maxB:
            self._init_rnd(M)
        result = super().learn()
        n_upd = self._static["n_upd"]
        self._rnd_steps += n_upd
        self._rnd_batches += 1 + n_upd
        return result

    def _alloc_static(self, M):
        net, E, B, S = self._net, self.n_epoch, self.batch_size, self.state_size
        cont = self.action_type == "continuous"
        n = net.n_actions
        nv = 2 * n if cont else n  # the column of v in a packed row; v_i follows it
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=self.device)
        z = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=self.device)
        n_upd = E * ((M + B - 1) // B)
        x_all = f(2 * M, S)
        st = dict(M=M, n_upd=n_upd, nv=nv, x_all=x_all,
                  tr={"state": x_all[:M], "next_state": x_all[M:], "action": f(M, n if cont else 1), "reward": f(M, 1), "done": f(M, 1)},
                  arange=torch.arange(M, dtype=torch.int64, device=self.device), idx=torch.zeros(E * M, dtype=torch.int64, device=self.device),
                  packed=f(2 * M, net.A), upto_v=f(2 * M, nv + 1), h0=f(2 * M, n), h1=f(2 * M, n) if cont else None, v=f(2 * M), v_i=f(2 * M),
                  logp_old=f(M, n if cont else 1), r_i=f(M, 1), zero=z(M, 1), adv_e=f(M, 1), adv_i=f(M, 1), ret=f(M, 1), ret_i=f(M, 1), adv=f(M, 1),
                  x_mb=f(B, S), heads_mb=f(B, net.A), grad_mb=z(B, net.A),
                  # rows 0 .. n_upd - 1: jh_rnd_ppo_loss_packed's; row n_upd: mean(ret), mean(ret_i)
                  stats=z(n_upd + 1, 8),
                  # the module's rows {r_i mean, 0, 0, mark}
                  rnd_stats=z(n_upd, 4))
        self._alloc_idx_lists(st, E * M)
        self._stats = st["stats"]
        return st

    def _enqueue_pre(self, st, captured=False):
        """rnd_ppo.py:102-166."""
        net, rnd, M, tr, cont = self._net, self._rnd_net, st["M"], st["tr"], self.action_type == "continuous"
        self.memory._store.gather(st["arange"], as_float=True, out={k: tr[k] for k in tr})
        rnd.obs_update(tr["next_state"])
        rnd.reward(tr["next_state"], st["r_i"])
        for o in range(0, 2 * M, net.maxB):
            net.forward(st["x_all"][o : o + net.maxB], 0, None, out=st["packed"][o : o + net.maxB])
        # (pi | v | v_i): first everything up to v as ONE head with v_i as its value, then the heads and v
        ops.heads_unpack(st["packed"], st["nv"] + 1, st["upto_v"], None, st["v_i"])
        ops.heads_unpack(st["packed"], net.n_actions, st["h0"], st["h1"], st["v"])
        if cont:
            ops.logp_continuous(st["h0"][:M], st["h1"][:M], tr["action"], out=st["logp_old"])
        else:
            ops.logp_discrete(st["h0"][:M], tr["action"], out=st["logp_old"])
        reward = st["zero"] if self.non_extrinsic else tr["reward"]  # reward *= 0.0 (rnd_ppo.py:113-114)
        done_i = st["zero"] if self.non_episodic else tr["done"]     # episodic_factor = 1.0 in the delta and in the scan (rnd_ppo.py:137-151)
        ops.gae(reward, tr["done"], st["v"][:M], st["v"][M:], self.n_step, self.gamma, self._lambda, False, out=(st["adv_e"], st["ret"]))
        ops.gae(st["r_i"], done_i, st["v_i"][:M], st["v_i"][M:], self.n_step, self.gamma_i, self._lambda, False, out=(st["adv_i"], st["ret_i"]))
        ops.rnd_adv_mix(st["adv_e"], st["adv_i"], st["ret"], st["ret_i"], self.n_step, self.extrinsic_coeff, self.intrinsic_coeff, self.use_standardization,
                        out=st["adv"], means=st["stats"][st["n_upd"]])

    def _enqueue_main(self, st):
        """rnd_ppo.py:168-266: the minibatch updates of all epochs (st["idx"] = the epochs' shuffles)."""
        net, rnd, M, B, tr, cont = self._net, self._rnd_net, st["M"], self.batch_size, st["tr"], self.action_type == "continuous"
        k = 0
        for e in range(self.n_epoch):
            for offset in range(0, M, B):
                b = min(B, M - offset)
                idx = st["idx"][e * M + offset : e * M + offset + b]
                x = st["x_mb"][:b]
                self.memory._store.gather(idx, names=["state"], as_float=True, out={"state": x})
                heads, grad = st["heads_mb"][:b], st["grad_mb"][:b]
                net.forward_keep(x, heads)
                ops.rnd_ppo_loss_packed(heads, net.n_actions, idx, tr["action"], st["adv"], st["ret"], st["ret_i"], st["v"][:M], st["v_i"][:M], st["logp_old"],
                                        self.epsilon_clip, self.vf_coef, self.ent_coef, grad, st["stats"][k], continuous=cont)
                net.backward(grad)
                net.optim_step("adam", max_norm=self.clip_grad_norm)
                rnd.update(tr["next_state"], idx, self.clip_grad_norm, stats=st["rnd_stats"][k])
                k += 1

    def _stat_tensors(self, st):
        return st["stats"], st["rnd_stats"]

    def _result(self, s, r, n_upd):
        return {"actor_loss": np.mean(s[:n_upd, 1]), "critic_e_loss": np.mean(s[:n_upd, 2]), "critic_i_loss": np.mean(s[:n_upd, 3]),
                "entropy_loss": np.mean(s[:n_upd, 4]), "r_i": np.mean(r[:n_upd, 0]), "max_ratio": float(s[:n_upd, 5].max()), "min_prob": float(s[:n_upd, 6].min()),
                "mean_ret": float(s[n_upd, 0]), "mean_ret_i": float(s[n_upd, 1])}

    # ---------------------------------------------------------------------------------- checkpoint
    def _sync_rnd_out(self):
        """Device statistics block -> the container's buffer-like Parameters and the batch norms' buffers."""
        blk = self._rnd_net.stats()
        with torch.no_grad():
            for k in _BLOCK_KEYS:
                mod, name = k.split(".")
                getattr(getattr(self.rnd, mod), name).copy_(torch.from_numpy(blk[k]))
            if self.batch_norm:
                for bn in _BN:
                    m = getattr(self.rnd, bn)
                    m.running_mean.copy_(torch.from_numpy(blk[bn + ".running_mean"]))
                    m.running_var.copy_(torch.from_numpy(blk[bn + ".running_var"]))
                    m.num_batches_tracked.fill_(self._rnd_batches)

    def _sync_rnd_in(self):
        """The container (after load_state_dict) -> the device statistics block and the batch counter."""
        sd = self.rnd.state_dict()
        self._rnd_net.set_stats({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
        if self.batch_norm:
            self._rnd_batches = int(self.rnd.bn1_predict_mlp.num_batches_tracked)

    def _resume_extra_attrs(self):
        d = super()._resume_extra_attrs()
        d["rnd_steps"], d["rnd_batches"] = int(self._rnd_steps), int(self._rnd_batches)
        return d

    def _resume_load_extra_attrs(self, d):
        super()._resume_load_extra_attrs(d)
        self._rnd_steps, self._rnd_batches = int(d.get("rnd_steps", self._rnd_steps)), int(d.get("rnd_batches", self._rnd_batches))

    def save(self, path):
        print(f"...Save model to {path}...")
        opt, params, _ = shadow_of(self._net, self._optim_config, self._lr_now)
        if self._adam_steps > 0:
            optim_state.fill(opt, params, self._adam_steps, *moments_of(self._net))
        export_views(self.rnd_optimizer, self._rnd_views, self._rnd_steps)  # the frozen and the buffer-like parameters never get a gradient: no views, no state
        self._sync_rnd_out()
        torch.save({"network": self.network.state_dict(), "rnd": self.rnd.state_dict(), "optimizer": opt.state_dict(), "rnd_optimizer": self.rnd_optimizer.state_dict()},
                   os.path.join(path, "ckpt"))

    def load(self, path):
        print(f"...Load model from {path}...")
        checkpoint = torch.load(os.path.join(path, "ckpt"), map_location=self.device, weights_only=False)
        self.network.load_state_dict(checkpoint["network"])
        opt, params, keys = shadow_of(self._net, self._optim_config, self._lr_now)
        opt.load_state_dict(checkpoint["optimizer"])
        self._adam_steps = load_moments(self._net, keys, opt, params)
        self._lr_now = float(opt.param_groups[0]["lr"])
        self._set_native_hyper(opt.param_groups[0], self._adam_steps)
        self.rnd.load_state_dict(checkpoint["rnd"])
        self.rnd_optimizer.load_state_dict(checkpoint["rnd_optimizer"])
        torch.cuda.current_stream().synchronize()
        self._sync_rnd_in()
        self._rnd_steps = steps = import_views(self.rnd_optimizer, self._rnd_views)
        d = self.rnd_optimizer.defaults
        self._rnd_net.set_hyper(self.rnd_optimizer.param_groups[0]["lr"], d["betas"][0], d["betas"][1], d["eps"], step=steps)
