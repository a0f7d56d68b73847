"""Agent factory with the reference's interface (core/agent/__init__.py:32-42): `Agent(name, **cfg)`.
Keys match the reference's auto-registered snake_case class names."""
from .base import BaseAgent
from .ddpg import DDPG
from .dqn import DQN, ApeX, Double, Multistep, PER
from .dueling import Dueling
from .icm_ppo import ICM_PPO
from .rnd_ppo import RND_PPO
from .iqn import IQN
from .mdqn import MDQN
from .miqn import MIQN
from .mpo import MPO
from .noisy import Noisy
from .ppo import PPO
from .qrdqn import QRDQN
from .r2d2 import R2D2
from .rainbow import C51, Rainbow
from .rainbow_iqn import RainbowIQN
from .reinforce import REINFORCE
from .sac import SAC
from .td3 import TD3
from .vmpo import VMPO

agent_dict = {"dqn": DQN, "double": Double, "multistep": Multistep, "per": PER, "ape_x": ApeX, "c51": C51, "rainbow": Rainbow, "ppo": PPO, "qrdqn": QRDQN, "m_dqn": MDQN, "iqn": IQN,
              "m_iqn": MIQN, "td3": TD3, "ddpg": DDPG, "sac": SAC, "vmpo": VMPO,
              "mpo": MPO, "noisy": Noisy, "dueling": Dueling, "icm_ppo": ICM_PPO, "rnd_ppo": RND_PPO, "r2d2": R2D2, "reinforce": REINFORCE, "rainbow_iqn": RainbowIQN}


def Agent(name, *args, **kwargs):
    if not isinstance(name, str):
        raise Exception("### name variable must be string! ###")
    key = name.lower()
    if key not in agent_dict:
        raise Exception(f"### can use only follows {list(agent_dict.keys())}")
    return agent_dict[key](*args, **kwargs)
