from .dqn import DQN


class Dueling(DQN):
    """core/agent/dueling.py:4-9: DQN on the dueling network; a `network` key is forced to "dueling", without one the assertion of the
    reference fails -- here "dueling" is the default, and anything else raises."""

    def __init__(self, *args, **kwargs):
        given = kwargs.get("network", "dueling")
        if given != "dueling":
            raise ValueError(f"the Dueling agent runs the 'dueling' network only (core/agent/dueling.py), got network={given!r}")
        kwargs["network"] = "dueling"
        super().__init__(*args, **kwargs)
