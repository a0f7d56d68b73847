import numpy as np
import torch

from ... import ops
from ..buffer import RolloutBuffer
from ..network import Network
from ..optimizer import Optimizer
from .base import BaseAgent
from .native_net import NativeNet, NativeValueNetMixin

MAX_ROWS = ops.REINFORCE_MAX_ROWS  # jh_reinforce_*: the rows of one learn()
MAX_ACTIONS = {"discrete": 64, "continuous": 32}  # logits | action dimensions per row the loss kernels loop over
REINFORCE_ELIGIBLE = ("REINFORCE runs on libjorldy_hip only: network in {discrete_policy, continuous_policy}, head 'mlp' with a scalar state_size or head 'cnn' "
                      "with a (C, H, W) state_size (H, W >= 36), hidden_size % 4 == 0, optim_config {'name': 'adam', lr, betas, eps}, "
                      f"2 <= action_size <= {MAX_ACTIONS['discrete']} (discrete) or 1 <= action_size <= {MAX_ACTIONS['continuous']} (continuous), row_capacity >= 1 "
                      "(config.reinforce.cartpole and its shapes); the multi head and data-parallel learners (grad_sync) are not available for this agent")


class PolicyNet(NativeNet):
    """`agent.network`: state_dict in the reference's keys (head.*, l, pi | mu, log_std: network/policy.py:23-55) over the library's flat bucket;
    calling it returns pi (discrete) or (mu, std) (continuous) like the reference module's forward."""

    @torch.no_grad()
    def raw(self, x):
        """The head's raw outputs [rows, A] (logits) or [rows, 2A] (mu_raw | log_std_raw), in slabs of the network's row capacity."""
        net = self._net
        x = x.contiguous()
        if x.dtype not in (torch.uint8, torch.float32):
            x = x.to(torch.float32)
        outs = [net.forward(x[o : o + net.maxB], self._which, None) for o in range(0, x.shape[0], net.maxB)]
        return (outs[0] if len(outs) == 1 else torch.cat(outs, 0)).view(-1, net.A)

    def __call__(self, x):
        out = self.raw(x)
        if self._net.kind == "pi":
            return torch.softmax(out, dim=-1)
        n = self._net.n_actions
        return torch.clamp(out[:, :n], min=-5.0, max=5.0), torch.tanh(out[:, n:]).exp()


class REINFORCE(NativeValueNetMixin, BaseAgent):
    """core/agent/reinforce.py:14-142 on the native engine.

      network       the discrete policy (head -> l -> pi, ops.RainbowNet kind "pi") or the Gaussian policy (head -> l -> mu | log_std, kind "gauss":
                    a q-network with 2A output rows), on the MLP or the Nature-CNN head; the reference's module draws the initial weights.
      act()         reinforce.py:66-81: softmax then multinomial / argmax; tanh(torch.normal(mu, std)) / tanh(mu).  Returns {"action"} only.
      learn()       memory.sample() -> jh_rbnet_forward_keep over the episode's T rows -> jh_reinforce_returns (the discounted scan over ALL rows
                    and the standardisation, in double) -> jh_reinforce_loss_discrete | _continuous (loss and head gradient) -> jh_rbnet_backward ->
                    Adam (no clipping: the reference has none).  It runs EAGERLY: T changes with every episode, so there is no hipGraph to
                    replay; the number of launches does not depend on T.  The loss is read back once, at the end.
      row capacity  an episode can outgrow the network object's row capacity (`row_capacity`, a library-only keyword): learn() then rebuilds
                    the object at twice the capacity (doubling until the rows fit) and carries parameters, both Adam moments and the hyper block
                    (lr, betas, eps, step count) across as they are -- bit-identical to an agent that started large enough.  More than
                    65536 rows in one learn() raise.
      process()     reinforce.py:115-126: store; learn only when transitions[0]["done"]; then the cosine lr decay.

    Departure on purpose: log pi is a log-softmax of the logits where the reference takes log(softmax) (as MPO's kernel).  save() / load() are
    the reference's {"network", "optimizer"}."""

    def __init__(self, state_size, action_size, hidden_size=512, network="discrete_policy", head="mlp", optim_config={"name": "adam"}, gamma=0.99,
                 use_standardization=True, run_step=1e6, lr_decay=True, device=None, row_capacity=1024, **kwargs):
        kinds = {"discrete_policy": "pi", "continuous_policy": "gauss"}
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        ok_state = (head == "mlp" and is_int(state_size)) or (head == "cnn" and not np.isscalar(state_size) and len(state_size) == 3
                                                              and all(is_int(v) for v in state_size) and min(state_size[1:]) >= 36)
        ok = (network in kinds and ok_state and is_int(hidden_size) and hidden_size > 0 and hidden_size % 4 == 0 and isinstance(optim_config, dict)
              and str(optim_config.get("name", "adam")).lower() == "adam" and set(optim_config) <= {"name", "lr", "betas", "eps"} and is_int(action_size)
              and (network != "discrete_policy" or 2 <= action_size <= MAX_ACTIONS["discrete"])
              and (network != "continuous_policy" or 1 <= action_size <= MAX_ACTIONS["continuous"])
              and is_int(row_capacity) and row_capacity >= 1 and kwargs.get("grad_sync") is None)
        if not ok:
            raise ValueError(f"{REINFORCE_ELIGIBLE}; got network={network!r}, head={head!r}, state_size={state_size!r}, hidden_size={hidden_size!r}, "
                             f"optim_config={optim_config!r}, action_size={action_size!r}, row_capacity={row_capacity!r}, grad_sync={kwargs.get('grad_sync')!r}")
        self.device = self._require_gpu(device)
        self.grad_sync = None
        self.action_type = network.split("_")[0]
        self.head, self.action_size, self.hidden_size = head, int(action_size), int(hidden_size)
        self.state_size = int(state_size) if head == "mlp" else [int(v) for v in state_size]
        self.gamma, self.use_standardization, self.run_step, self.lr_decay = gamma, use_standardization, run_step, lr_decay
        torch_net = Network(network, self.state_size, self.action_size, D_hidden=self.hidden_size, head=head)  # the reference's initialisation, drawn on the host
        self._kind = kinds[network]
        self._net = self._build(int(row_capacity))
        self._net.import_state(torch_net.state_dict())
        self.network = PolicyNet(self._net, 0)
        self._optim_config = dict(optim_config)
        self._opt_name = "adam"
        d = Optimizer(**optim_config, params=[torch.nn.Parameter(torch.zeros(1))]).defaults
        self._lr0, self._lr_now, self._adam_steps = float(d["lr"]), float(d["lr"]), 0
        self._set_native_hyper(d, 0)
        self.optimizer = None
        self.memory = RolloutBuffer(device=self.device)
        self._stats = torch.zeros(len(ops.REINFORCE_STATS), dtype=torch.float32, device=self.device)
        self._learn_graphs = ops.LearnGraphs("REINFORCE.learn()")  # never captures: T changes with every episode
        self._last = None  # the device tensors of the last learn(): out, ret, grad

    # ---------------------------------------------------------------------------------- the network object and its row capacity
    def _build(self, rows):
        return ops.RainbowNet(self.state_size, self.action_size, 1, self.hidden_size, self.head, rows, self.device, kind=self._kind)

    row_capacity = property(lambda self: self._net.maxB)

    def _ensure_rows(self, rows):
        """A network object that holds `rows` rows: the present one, or a new one at twice the capacity (doubled until the rows fit) with the
        parameters, both moments and the hyper block of the old one, bit for bit."""
        old = self._net
        if rows <= old.maxB:
            return
        cap = old.maxB
        while cap < rows:
            cap *= 2
        new = self._build(cap)
        assert new.n_params == old.n_params
        hyper = lambda net: ops._wrap_device(net.hyper_ptr(), (16,), torch.float32, self.device, owner=net)
        with torch.no_grad():
            for dst, src in ((new.params, old.params), (new.target, old.target), (new.m, old.m), (new.v, old.v), (hyper(new), hyper(old))):
                dst.copy_(src)
        torch.cuda.current_stream().synchronize()  # `old` is destroyed when it goes out of scope
        self._net = new
        self.network = PolicyNet(new, 0)
        self.__dict__.pop("_actbuf", None)

    # ---------------------------------------------------------------------------------- act
    @torch.no_grad()
    def act(self, state, training=True):
        """reinforce.py:66-81."""
        self.network.train(training)
        if self.action_type == "continuous":
            mu, std = self.network(self.as_tensor(state))
            z = torch.normal(mu, std) if training else mu
            action = torch.tanh(z)
        else:
            pi = self.network(self.as_tensor(state))
            action = torch.multinomial(pi, 1) if training else torch.argmax(pi, dim=-1, keepdim=True)
        return {"action": action.cpu().numpy()}

    # ---------------------------------------------------------------------------------- learn
    def learn(self):
        """reinforce.py:83-113.  Eager: no hipGraph, T is the episode's length."""
        T = int(self.memory.size)
        if T > MAX_ROWS:
            raise ValueError(f"REINFORCE.learn(): {T} rows in one learn, more than the {MAX_ROWS} the return scan and the loss kernels take (jh_reinforce_*)")
        if T < 1:
            raise ValueError("REINFORCE.learn(): the rollout is empty")
        self._ensure_rows(T)
        net = self._net
        tr = self.memory.sample(as_float=self._as_float())
        state = tr["state"].contiguous()
        out = torch.empty(T, net.A, 1, dtype=torch.float32, device=self.device)
        net.forward_keep(state, out)
        ret = ops.reinforce_returns(tr["reward"], self.gamma, self.use_standardization)
        loss_fn = ops.reinforce_loss_continuous if self.action_type == "continuous" else ops.reinforce_loss_discrete
        grad, _ = loss_fn(out.view(T, net.A), tr["action"], ret, stats=self._stats)
        net.backward(grad)
        net.optim_step("adam", None)
        self._adam_steps += 1
        self._last = dict(T=T, out=out.view(T, net.A), ret=ret, grad=grad)
        return {"loss": float(self._read_stats(self._stats)[0][0])}

    def learning_rate_decay(self, step, optimizers=None, mode="cosine"):
        self._native_lr_decay(step, mode)

    def process(self, transitions, step):
        """reinforce.py:115-126."""
        result = {}
        self.memory.store(transitions)
        if transitions[0]["done"]:
            result = self.learn()
            if self.lr_decay:
                self.learning_rate_decay(step)
        return result

    # ---------------------------------------------------------------------------------- checkpoint
    def save(self, path):
        self._native_save(path)

    def load(self, path):
        self.target_network = self.network  # (_native_load mirrors the online weights into the family's target network: there is none here)
        try:
            self._native_load(path)
        finally:
            del self.target_network
