"""Parameter containers of the hot-path networks: the reference's parameter names, shapes, registration order (= `state_dict`
layout, so checkpoints and `sync_in/out` payloads interchange) and initialisation -- and nothing else.  There is NO forward here:
every forward / backward / optimizer step of the product runs in libjorldy_hip (ops.PPONet, ops.RainbowNet); these modules only
provide the initial weights and, for PPO, the nn.Parameter views of the native flat bucket that `state_dict()` / the torch
checkpoint format need.  (The forward-capable restatement that the parity tests evaluate in float64 lives in tests/mirror.)
  head.mlp / head.cnn          core/network/head.py:6-61
  discrete_q_network           core/network/q_network.py:8-20
  discrete_policy_value        core/network/policy_value.py:8-22
  continuous_policy_value      core/network/policy_value.py:38-57
  discrete_policy_separate_value / continuous_policy_separate_value   core/network/policy_value.py:25-35, 60-70 (a second value head v_i)
  dueling                      core/network/dueling.py:8-35
  rainbow                      core/network/rainbow.py:8-94 (+ utils.py:55-107 noisy linear)
  noisy                        core/network/noisy.py:8-50 (+ utils.py:89-107 init_weights)
  iqn                          core/network/iqn.py:9-47
  rainbow_iqn                  core/network/rainbow_iqn.py:9-40
  deterministic_policy         core/network/policy.py:8-20
  continuous_q_network         core/network/q_network.py:23-39
  continuous_policy            core/network/policy.py:38-55
  discrete_policy              core/network/policy.py:23-35
  icm_mlp                      core/network/icm.py:153-188 (+ utils.py:6-24 reward filter, running moments)
  rnd_mlp                      core/network/rnd.py:13-35, 167-203 (predictor and frozen target)
  r2d2                         core/network/r2d2.py:8-26
"""
import torch


def orthogonal_init(layer, nonlinearity="relu"):
    """core/network/utils.py:110-124."""
    if isinstance(nonlinearity, str):
        gain = 0.01 if nonlinearity == "policy" else torch.nn.init.calculate_gain(nonlinearity)
    else:
        gain = nonlinearity
    for l in layer if isinstance(layer, list) else [layer]:
        torch.nn.init.orthogonal_(l.weight.data, gain)
        torch.nn.init.zeros_(l.bias.data)


class _Container(torch.nn.Module):
    def forward(self, *args, **kwargs):
        raise RuntimeError(f"{type(self).__name__} is a parameter container: the product computes in libjorldy_hip (ops.PPONet / ops.RainbowNet), "
                           "not in torch modules")


class MLP(_Container):
    def __init__(self, D_in, D_hidden=512):
        super().__init__()
        self.l = torch.nn.Linear(D_in, D_hidden)
        self.D_head_out = D_hidden
        orthogonal_init(self.l)


class CNN(_Container):
    """Nature-CNN head (head.py:21-61)."""

    def __init__(self, D_in, D_hidden=512):
        super().__init__()
        assert D_in[1] >= 36 and D_in[2] >= 36
        self.conv1 = torch.nn.Conv2d(D_in[0], 32, kernel_size=8, stride=4)
        d1 = ((D_in[1] - 8) // 4 + 1, (D_in[2] - 8) // 4 + 1)
        self.conv2 = torch.nn.Conv2d(32, 64, kernel_size=4, stride=2)
        d2 = ((d1[0] - 4) // 2 + 1, (d1[1] - 4) // 2 + 1)
        self.conv3 = torch.nn.Conv2d(64, 64, kernel_size=3, stride=1)
        d3 = (d2[0] - 3 + 1, d2[1] - 3 + 1)
        self.D_head_out = 64 * d3[0] * d3[1]
        for layer in (self.conv1, self.conv2, self.conv3):
            orthogonal_init(layer)


head_dict = {"mlp": MLP, "cnn": CNN}


class BaseNetwork(_Container):
    def __init__(self, D_in, D_hidden, head):
        super().__init__()
        assert head in head_dict, f"head {head!r} is outside the hot path (have {list(head_dict)})"
        self.head = head_dict[head](D_in, D_hidden)


class DiscreteQ_Network(BaseNetwork):
    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.q = torch.nn.Linear(D_hidden, D_out)
        orthogonal_init(self.l)
        orthogonal_init(self.q, "linear")


class DiscretePolicyValue(BaseNetwork):
    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.pi = torch.nn.Linear(D_hidden, D_out)
        self.v = torch.nn.Linear(D_hidden, 1)
        orthogonal_init(self.l)
        orthogonal_init(self.pi, "policy")
        orthogonal_init(self.v, "linear")


class ContinuousPolicyValue(BaseNetwork):
    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.mu = torch.nn.Linear(D_hidden, D_out)
        self.log_std = torch.nn.Linear(D_hidden, D_out)
        self.v = torch.nn.Linear(D_hidden, 1)
        orthogonal_init(self.l)
        orthogonal_init(self.mu, "linear")
        orthogonal_init(self.log_std, "tanh")
        orthogonal_init(self.v, "linear")


class DiscretePolicySeparateValue(DiscretePolicyValue):
    """RND-PPO's discrete net (policy_value.py:25-35): one more value head v_i for the intrinsic return; v and v_i are re-drawn with gain 0.01
    after the parent's initialisation, in this order, so one torch.manual_seed gives the reference's weights."""

    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_out, D_hidden, head)
        self.v_i = torch.nn.Linear(D_hidden, 1)
        orthogonal_init([self.v, self.v_i], 0.01)


class ContinuousPolicySeparateValue(ContinuousPolicyValue):
    """RND-PPO's continuous net (policy_value.py:60-70), as DiscretePolicySeparateValue."""

    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_out, D_hidden, head)
        self.v_i = torch.nn.Linear(D_hidden, 1)
        orthogonal_init([self.v, self.v_i], 0.01)


class Dueling(BaseNetwork):
    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l1_a = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.l1_v = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.l2_a = torch.nn.Linear(D_hidden, D_out)
        self.l2_v = torch.nn.Linear(D_hidden, 1)
        orthogonal_init([self.l1_a, self.l1_v])
        orthogonal_init([self.l2_a, self.l2_v], "linear")


class R2D2(BaseNetwork):
    """Recurrent dueling network (r2d2.py:8-26): head -> cat[x, prev_action_onehot] -> LSTM(D_head_out + D_out -> D_hidden) -> relu(l) ->
    dueling streams.  torch.nn.LSTM is held for its four parameters (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0; gate order i, f,
    g, o) and their default initialisation; orthogonal_init runs on the four stream layers only, as in the reference."""

    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.D_hidden = D_hidden
        self.lstm = torch.nn.LSTM(input_size=self.head.D_head_out + D_out, hidden_size=D_hidden, batch_first=True)
        self.l = torch.nn.Linear(D_hidden, D_hidden)
        self.l1_a = torch.nn.Linear(D_hidden, D_hidden)
        self.l1_v = torch.nn.Linear(D_hidden, D_hidden)
        self.l2_a = torch.nn.Linear(D_hidden, D_out)
        self.l2_v = torch.nn.Linear(D_hidden, 1)
        orthogonal_init([self.l1_a, self.l1_v])
        orthogonal_init([self.l2_a, self.l2_v], "linear")


def _noisy_params(shape, noise_type):
    """core/network/utils.py:89-107."""
    if noise_type == "factorized":
        mu_init, sig_init = 1.0 / (shape[0] ** 0.5), 0.5 / (shape[0] ** 0.5)
    else:
        mu_init, sig_init = (3.0 / shape[0]) ** 0.5, 0.017
    mu_w = torch.nn.Parameter(torch.empty(shape).uniform_(-mu_init, mu_init))
    sig_w = torch.nn.Parameter(torch.full(shape, sig_init))
    mu_b = torch.nn.Parameter(torch.empty(shape[1]).uniform_(-mu_init, mu_init))
    sig_b = torch.nn.Parameter(torch.full((shape[1],), sig_init))
    return mu_w, sig_w, mu_b, sig_b


class Rainbow(BaseNetwork):
    """Dueling + noisy + categorical head (rainbow.py:8-94)."""

    def __init__(self, D_in, D_out, N_atom, noise_type="factorized", D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.D_out, self.N_atom, self.noise_type = D_out, N_atom, noise_type
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.mu_w_a1, self.sig_w_a1, self.mu_b_a1, self.sig_b_a1 = _noisy_params((D_hidden, D_hidden), noise_type)
        self.mu_w_v1, self.sig_w_v1, self.mu_b_v1, self.sig_b_v1 = _noisy_params((D_hidden, D_hidden), noise_type)
        self.mu_w_a2, self.sig_w_a2, self.mu_b_a2, self.sig_b_a2 = _noisy_params((D_hidden, N_atom * D_out), noise_type)
        self.mu_w_v2, self.sig_w_v2, self.mu_b_v2, self.sig_b_v2 = _noisy_params((D_hidden, N_atom), noise_type)
        orthogonal_init(self.l)


def _init_weights(shape, noise_type):
    """core/network/utils.py:89-107 call for call: mu_w, mu_b, sig_w, sig_b are each filled by a `uniform_` in this order -- the constant sigma
    fills draw from the generator too, so the next layer's mu sees the reference's stream."""
    if noise_type == "factorized":
        mu_init, sig_init = 1.0 / (shape[0] ** 0.5), 0.5 / (shape[0] ** 0.5)
    else:
        mu_init, sig_init = (3.0 / shape[0]) ** 0.5, 0.017
    mu_w, sig_w = torch.nn.Parameter(torch.empty(shape)), torch.nn.Parameter(torch.empty(shape))
    mu_b, sig_b = torch.nn.Parameter(torch.empty(shape[1])), torch.nn.Parameter(torch.empty(shape[1]))
    mu_w.data.uniform_(-mu_init, mu_init)
    mu_b.data.uniform_(-mu_init, mu_init)
    sig_w.data.uniform_(sig_init, sig_init)
    sig_b.data.uniform_(sig_init, sig_init)
    return mu_w, sig_w, mu_b, sig_b


class Noisy(BaseNetwork):
    """NoisyNet Q-network (noisy.py:8-20): head -> noisy(D_head_out -> D_hidden) -> noisy(D_hidden -> D_out)."""

    def __init__(self, D_in, D_out, noise_type="factorized", D_hidden=512, head="mlp"):
        assert noise_type in ["independent", "factorized"]
        super().__init__(D_in, D_hidden, head)
        self.noise_type = noise_type
        self.mu_w1, self.sig_w1, self.mu_b1, self.sig_b1 = _init_weights((self.head.D_head_out, D_hidden), noise_type)
        self.mu_w2, self.sig_w2, self.mu_b2, self.sig_b2 = _init_weights((D_hidden, D_out), noise_type)


class IQN(BaseNetwork):
    """Implicit quantile network (iqn.py:9-24).  The reference's orthogonal_init call names sample_embed twice and state_embed never
    (iqn.py:23): state_embed keeps nn.Linear's default initialisation, and so it does here."""

    def __init__(self, D_in, D_out, D_em=64, N_sample=64, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.N_sample, self.D_em = N_sample, D_em
        self.state_embed = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.sample_embed = torch.nn.Linear(D_em, D_hidden)
        self.l1 = torch.nn.Linear(D_hidden, D_hidden)
        self.l2 = torch.nn.Linear(D_hidden, D_hidden)
        self.q = torch.nn.Linear(D_hidden, D_out)
        orthogonal_init([self.sample_embed, self.sample_embed, self.l1, self.l2])
        orthogonal_init(self.q, "linear")


class RainbowIQN(BaseNetwork):
    """IQN's trunk under Rainbow's noisy dueling tail with one support (rainbow_iqn.py:9-40).  D_hidden is the caller's here; as in IQN the
    orthogonal_init call names sample_embed twice and state_embed never (rainbow_iqn.py:40).  Own parameters (the 16 noisy tensors) come
    first in state_dict(), the submodules after."""

    def __init__(self, D_in, D_out, D_em, N_sample, noise_type, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.D_out, self.noise_type, self.N_sample, self.D_em = D_out, noise_type, N_sample, D_em
        self.state_embed = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.sample_embed = torch.nn.Linear(D_em, D_hidden)
        self.l1 = torch.nn.Linear(D_hidden, D_hidden)
        self.l2 = torch.nn.Linear(D_hidden, D_hidden)
        self.mu_w_a1, self.sig_w_a1, self.mu_b_a1, self.sig_b_a1 = _init_weights((D_hidden, D_hidden), noise_type)
        self.mu_w_v1, self.sig_w_v1, self.mu_b_v1, self.sig_b_v1 = _init_weights((D_hidden, D_hidden), noise_type)
        self.mu_w_a2, self.sig_w_a2, self.mu_b_a2, self.sig_b_a2 = _init_weights((D_hidden, D_out), noise_type)
        self.mu_w_v2, self.sig_w_v2, self.mu_b_v2, self.sig_b_v2 = _init_weights((D_hidden, 1), noise_type)
        orthogonal_init([self.sample_embed, self.sample_embed, self.l1, self.l2])


class DeterministicPolicy(BaseNetwork):
    """The actor of TD3 / DDPG (policy.py:8-20): head -> relu(l) -> tanh(pi)."""

    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.pi = torch.nn.Linear(D_hidden, D_out)
        orthogonal_init(self.l)
        orthogonal_init(self.pi, "tanh")


class DiscretePolicy(BaseNetwork):
    """The actor of discrete MPO (policy.py:23-35): head -> relu(l) -> softmax(pi).  The shape of discrete_q_network with the last layer
    named pi and initialised with the policy gain 0.01."""

    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.pi = torch.nn.Linear(D_hidden, D_out)
        orthogonal_init(self.l)
        orthogonal_init(self.pi, "policy")


class ContinuousPolicy(BaseNetwork):
    """The actor of SAC (policy.py:38-55): head -> relu(l) -> (clamp(mu, -5, 5), exp(tanh(log_std)))."""

    def __init__(self, D_in, D_out, D_hidden=512, head="mlp"):
        super().__init__(D_in, D_hidden, head)
        self.l = torch.nn.Linear(self.head.D_head_out, D_hidden)
        self.mu = torch.nn.Linear(D_hidden, D_out)
        self.log_std = torch.nn.Linear(D_hidden, D_out)
        orthogonal_init(self.l)
        orthogonal_init(self.mu, "linear")
        orthogonal_init(self.log_std, "tanh")


class ContinuousQ_Network(BaseNetwork):
    """The critic of TD3 / DDPG (q_network.py:23-39): [head(state) | relu(e(action))] -> relu(l) -> q.  The reference's argument order:
    head comes before D_hidden."""

    def __init__(self, D_in1, D_in2, head="mlp", D_hidden=512):
        super().__init__(D_in1, D_hidden, head)
        self.e = torch.nn.Linear(D_in2, D_hidden)
        self.l = torch.nn.Linear(D_hidden + self.head.D_head_out, D_hidden)
        self.q = torch.nn.Linear(D_hidden, 1)
        orthogonal_init(self.e)
        orthogonal_init(self.l)
        orthogonal_init(self.q, "linear")


class RunningMeanStd(_Container):
    """core/network/utils.py:18-24: running mean, variance and count as Parameters without gradient."""

    def __init__(self, shape, epsilon=1e-4):
        super().__init__()
        self.mean = torch.nn.Parameter(torch.zeros(shape), requires_grad=False)
        self.var = torch.nn.Parameter(torch.zeros(shape), requires_grad=False)
        self.count = torch.nn.Parameter(torch.tensor(epsilon), requires_grad=False)


class RewardForwardFilter(_Container):
    """core/network/utils.py:6-10: the discounted sum of intrinsic rewards per worker."""

    def __init__(self, gamma, num_workers):
        super().__init__()
        self.rewems = torch.nn.Parameter(torch.zeros(num_workers), requires_grad=False)
        self.gamma = gamma


class ICM_MLP(_Container):
    """ICM-PPO's curiosity module (icm.py:153-188): module names, registration order and torch's default initialisation as the reference's,
    so its state_dict has the reference's 34 keys (25 without batch norm) and, after the same torch.manual_seed, the reference's weights.
    The feature size is 256 whatever D_hidden says (icm.py:181)."""

    def __init__(self, D_in, D_out, num_workers, gamma, eta, action_type, ri_normalize=True, obs_normalize=True, batch_norm=True, D_hidden=256):
        super().__init__()
        assert action_type in ("discrete", "continuous")
        self.D_in, self.D_out, self.num_workers, self.eta, self.action_type = D_in, D_out, num_workers, eta, action_type
        self.rms_obs = RunningMeanStd(D_in)
        self.rms_ri = RunningMeanStd(1)
        self.rff = RewardForwardFilter(gamma, num_workers)
        self.obs_normalize, self.ri_normalize, self.batch_norm = obs_normalize, ri_normalize, batch_norm
        feature_size = 256
        a = 1 if action_type == "discrete" else D_out
        self.fc1 = torch.nn.Linear(D_in, D_hidden)
        self.fc2 = torch.nn.Linear(D_hidden, feature_size)
        self.forward_fc1 = torch.nn.Linear(feature_size + a, D_hidden)
        self.forward_fc2 = torch.nn.Linear(D_hidden + a, feature_size)
        self.inverse_fc1 = torch.nn.Linear(2 * feature_size, D_hidden)
        self.inverse_fc2 = torch.nn.Linear(D_hidden, D_out)
        if batch_norm:
            self.bn1 = torch.nn.BatchNorm1d(D_hidden)
            self.bn2 = torch.nn.BatchNorm1d(feature_size)
            self.bn1_next = torch.nn.BatchNorm1d(D_hidden)


class RND_MLP(_Container):
    """RND-PPO's distillation module (rnd.py:173-203): module names, registration order and initialisation (orthogonal with the ReLU gain on
    the four linear layers, predictor first) as the reference's, so its state_dict has the reference's 35 keys (15 without batch norm) and,
    after the same torch.manual_seed, the reference's weights.  Every parameter whose name contains "target" is frozen -- the target's batch
    norm affine parameters too.  The feature size is 256 whatever D_hidden says (rnd.py:196)."""

    def __init__(self, D_in, D_out, num_workers, gamma_i, ri_normalize=True, obs_normalize=True, batch_norm=True, D_hidden=256):
        super().__init__()
        self.D_in, self.D_out, self.num_workers = D_in, D_out, num_workers
        self.rms_obs = RunningMeanStd(D_in)
        self.rms_ri = RunningMeanStd(1)
        self.rff = RewardForwardFilter(gamma_i, num_workers)
        self.obs_normalize, self.ri_normalize, self.batch_norm = obs_normalize, ri_normalize, batch_norm
        feature_size = 256
        self.fc1_predict_mlp = torch.nn.Linear(D_in, D_hidden)
        self.fc2_predict_mlp = torch.nn.Linear(D_hidden, feature_size)
        self.fc1_target_mlp = torch.nn.Linear(D_in, D_hidden)
        self.fc2_target_mlp = torch.nn.Linear(D_hidden, feature_size)
        orthogonal_init([self.fc1_predict_mlp, self.fc2_predict_mlp, self.fc1_target_mlp, self.fc2_target_mlp])
        if batch_norm:
            self.bn1_predict_mlp = torch.nn.BatchNorm1d(D_hidden)
            self.bn2_predict_mlp = torch.nn.BatchNorm1d(feature_size)
            self.bn1_target_mlp = torch.nn.BatchNorm1d(D_hidden)
            self.bn2_target_mlp = torch.nn.BatchNorm1d(feature_size)
        for name, param in self.named_parameters():
            if "target" in name:
                param.requires_grad = False


network_dict = {
    "discrete_q_network": DiscreteQ_Network,
    "discrete_policy_value": DiscretePolicyValue,
    "continuous_policy_value": ContinuousPolicyValue,
    "discrete_policy_separate_value": DiscretePolicySeparateValue,
    "continuous_policy_separate_value": ContinuousPolicySeparateValue,
    "dueling": Dueling,
    "rainbow": Rainbow,
    "noisy": Noisy,
    "iqn": IQN,
    "rainbow_iqn": RainbowIQN,
    "deterministic_policy": DeterministicPolicy,
    "continuous_q_network": ContinuousQ_Network,
    "continuous_policy": ContinuousPolicy,
    "discrete_policy": DiscretePolicy,
    "icm_mlp": ICM_MLP,
    "rnd_mlp": RND_MLP,
    "r2d2": R2D2,
}


def Network(name, *args, **kwargs):
    """core/network/__init__.py:30-41 factory (hot-path networks only)."""
    if not isinstance(name, str):
        raise Exception("### name variable must be string! ###")
    key = name.lower()
    if key not in network_dict:
        raise Exception(f"### can use only follows {list(network_dict.keys())}")
    return network_dict[key](*args, **kwargs)
