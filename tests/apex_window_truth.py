"""Float64 restatement of what Ape-X's device-resident actors compute: the network of both kinds, and the n-step window with the
actor-side priority as one `deque` per env that follows ApeX.interact_callback (core/agent/dqn.py) line for line."""
from collections import deque

import numpy as np
import torch


def q_values(sd, kind, x):
    """network(x) from a state_dict, in the dtype of its tensors (float64 truth, or torch's CPU float32 beside it)."""
    lin = lambda name, v: v @ sd[name + ".weight"].T + sd[name + ".bias"]
    h = torch.relu(lin("head.l", torch.as_tensor(x, dtype=sd["head.l.weight"].dtype)))
    if kind == "discrete_q_network":
        return lin("q", torch.relu(lin("l", h)))
    a, v = lin("l2_a", torch.relu(lin("l1_a", h))), lin("l2_v", torch.relu(lin("l1_v", h)))
    return v + a - a.mean(-1, keepdim=True)


class Windows:
    def __init__(self, W, n_step, gamma):
        self.n, self.gamma = n_step, gamma
        self.buf = [deque(maxlen=n_step + 1) for _ in range(W)]

    def push(self, state, action, reward, done, q):
        """One timestep of all envs ([W, ...] arrays; reward, done, q in float64) -> [emitted row or None per env]."""
        out = []
        for w, buf in enumerate(self.buf):
            buf.append({"state": state[w], "action": action[w], "reward": float(reward[w]), "done": float(done[w]), "q": float(q[w])})
            row = None
            if len(buf) == buf.maxlen:
                row = {"state": buf[0]["state"], "action": buf[0]["action"], "next_state": buf[-1]["state"]}
                for key in ("reward", "done"):
                    row[key] = np.stack([t[key] for t in buf][:-1])
                target_q = buf[-1]["q"]
                for i in reversed(range(self.n)):
                    target_q = buf[i]["reward"] + (1 - buf[i]["done"]) * self.gamma * target_q
                row["priority"] = abs(target_q - buf[0]["q"])
            out.append(row)
        return out
