"""The float64 window helper of the device-actor tests against ApeX.interact_callback itself on a short random trace."""
import types
from collections import deque

import numpy as np
import pytest

import apex_window_truth as AW


@pytest.mark.parametrize("n_step", [1, 3, 8])
def test_helper_follows_interact_callback(n_step):
    from jorldy_amd.core.agent.dqn import ApeX

    rng, W, gamma = np.random.RandomState(n_step), 3, 0.99
    ours = AW.Windows(W, n_step, gamma)
    agents = [types.SimpleNamespace(tmp_buffer=deque(maxlen=n_step + 1), n_step=n_step, gamma=gamma) for _ in range(W)]
    emitted = 0
    for t in range(2 * n_step + 5):
        s, a = rng.randn(W, 4), rng.randint(0, 2, size=W)
        r, d, q = rng.choice([0.1, -1.0], size=W), (rng.rand(W) < 0.3).astype(np.float64), rng.randn(W)
        rows = ours.push(s, a, r, d, q)
        for w in range(W):
            ref = ApeX.interact_callback(agents[w], {"state": s[None, w], "action": a[None, None, w], "reward": r[None, None, w], "next_state": s[None, w] + 1,
                                                     "done": d[None, None, w], "q": q[None, None, w]})
            assert (rows[w] is None) == (not ref) == (t < n_step)
            if ref:
                emitted += 1
                for k in ("state", "action", "next_state"):
                    assert np.array_equal(np.asarray(ref[k]).reshape(-1), np.asarray(rows[w][k]).reshape(-1)), k
                for k in ("reward", "done"):
                    assert ref[k].shape == (1, n_step, 1) and np.array_equal(ref[k].reshape(-1), rows[w][k]), k
                assert float(ref["priority"].reshape(-1)[0]) == rows[w]["priority"]
    assert emitted == W * (n_step + 5)
