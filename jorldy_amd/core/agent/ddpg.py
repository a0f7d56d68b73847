import numpy as np
import torch

from .td3 import _ELIGIBLE, DeterministicActorCritic

DDPG_ELIGIBLE = _ELIGIBLE.format(name="DDPG", configs="config.ddpg x mujoco / pendulum / cartpole / hopper_mlagent")


class OUNoise:
    """The Ornstein-Uhlenbeck exploration state X [1, A] (core/agent/utils.py:8-24).  One step moves X by theta (mu - X) + sigma * n with n a
    single standard normal from numpy's global generator -- one draw for ALL action dimensions, len(X) being 1 -- so X, float32 until
    then, is float64 from the first step on (numpy's promotion with the float64 draw).  The same draws in the same order as the reference."""

    def __init__(self, action_size, mu, theta, sigma):
        self.mu, self.theta, self.sigma = mu, theta, sigma
        self.X = np.full((1, action_size), mu, dtype=np.float32)

    def sample(self):
        n = np.random.randn(self.X.shape[0])
        pull = self.theta * (self.mu - self.X)
        self.X = self.X + (pull + self.sigma * n)
        return self.X


class DDPG(DeterministicActorCritic):
    """core/agent/ddpg.py:14-211: TD3's machinery with one critic, no target noise and no delay: every learn() is a critic update and an
    actor update (one hipGraph), Ornstein-Uhlenbeck exploration noise, and the soft target update in process() on every call once learning
    has begun."""

    N_CRITICS = 1
    ELIGIBLE = DDPG_ELIGIBLE
    TARGET_NOISE = False
    CKPT_KEYS = (("actor", "actor", "net"), ("actor_optimizer", "actor", "opt"), ("critic", "critic1", "net"), ("critic_optimizer", "critic1", "opt"))  # ddpg.py:183-188

    def __init__(self, state_size, action_size, hidden_size=512, actor="deterministic_policy", critic="continuous_q_network", head="mlp",
                 optim_config={"actor": "adam", "critic": "adam", "actor_lr": 5e-4, "critic_lr": 1e-3}, gamma=0.99, buffer_size=50000, batch_size=128,
                 start_train_step=2000, tau=1e-3, run_step=1e6, lr_decay=True, mu=0, theta=1e-3, sigma=2e-3, device=None, use_graph=True, **kwargs):
        self._init_common(state_size, action_size, hidden_size, actor, critic, head, optim_config, gamma, buffer_size, batch_size, start_train_step, tau, run_step,
                          lr_decay, device, use_graph, ("online:actor", "online:critic", "target:actor", "target:critic"))  # ddpg.py:74-87
        self.actor_loss = 0.0
        self.OU = OUNoise(action_size, mu, theta, sigma)

    @torch.no_grad()
    def act(self, state, training=True):
        """ddpg.py:109-115: only the noise is clipped, not the action."""
        self.actor.train(training)
        mu = self._actor_np(state)
        action = mu + self.OU.sample().clip(-1.0, 1.0) if training else mu
        return {"action": action}

    def learn(self):
        s = self._learn_stats(True, False)
        self.actor_loss = float(s[4])
        self.num_learn += 1
        return {"critic_loss": float(s[0]), "actor_loss": self.actor_loss, "max_Q": float(s[2])}

    def process(self, transitions, step):
        """ddpg.py:165-179."""
        result = {}
        self._store(transitions)
        self.time_t = step
        if self.memory.size >= self.batch_size and step >= self.start_train_step:
            result = self.learn()
            if self.lr_decay:
                self.learning_rate_decay(step)
        if self.num_learn > 0:
            self.update_target_soft()
        return result

    def _resume_extra_attrs(self):
        return {"ou_x": np.asarray(self.OU.X, dtype=np.float64).tolist(), "ou_dtype": str(self.OU.X.dtype)}

    def _resume_load_extra_attrs(self, d):
        if "ou_x" in d:
            self.OU.X = np.asarray(d["ou_x"], dtype=np.dtype(d["ou_dtype"]))
