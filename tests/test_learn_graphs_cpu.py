"""ops.LearnGraphs, the capture-and-replay lifecycle every agent's learn() goes through, on the CPU: a counting fake stands in for
torch.cuda.CUDAGraph, a no-op for torch.cuda.synchronize, and ops.graph_capture is a context manager that yields or raises."""
import contextlib

import pytest
import torch

from jorldy_amd import ops


class FakeGraph:
    made = []

    def __init__(self):
        self.replays = 0
        FakeGraph.made.append(self)

    def replay(self):
        self.replays += 1


class Body:
    def __init__(self):
        self.runs = 0

    def __call__(self):
        self.runs += 1


@pytest.fixture
def fake(monkeypatch):
    """-> a dict whose "raise" entry makes the N-th capture from now (1-based) raise that exception; "captures" counts the attempts."""
    FakeGraph.made = []
    ctl = {"raise": {}, "captures": 0}

    @contextlib.contextmanager
    def capture(g):
        assert isinstance(g, FakeGraph)
        ctl["captures"] += 1
        if ctl["captures"] in ctl["raise"]:
            raise ctl["raise"][ctl["captures"]]
        yield

    monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    monkeypatch.setattr(ops, "graph_capture", capture)
    monkeypatch.setitem(ops._PROF, "lib", False)
    return ctl


def replays():
    return sum(g.replays for g in FakeGraph.made)


def test_one_key_eager_capture_replay(fake):
    lg, body = ops.LearnGraphs("X.learn()"), Body()
    assert [lg.run("k", body) for _ in range(4)] == [False, True, True, True]
    assert body.runs == 2, "once eagerly, once inside the capture"
    assert fake["captures"] == 1 and replays() == 3
    assert lg.last is lg.graphs["k"] and set(lg.graphs) == {"k"}


def test_shared_and_per_key_warm(fake):
    shared, a, b = ops.LearnGraphs("X.learn()"), Body(), Body()
    assert shared.run("a", a, warm_key="w") is False
    assert shared.run("b", b, warm_key="w") is True, "a shared warm key: the second variant is captured on its first call"
    assert b.runs == 1 and set(shared.graphs) == {"b"}
    own, a, b = ops.LearnGraphs("X.learn()"), Body(), Body()
    assert own.run("a", a) is False
    assert own.run("b", b) is False, "a warm key per key: the second key runs eagerly first"
    assert not own.graphs
    assert own.run("b", b) is True and own.run("a", a) is True and set(own.graphs) == {"a", "b"}


def test_never_eligible_only_warms(fake):
    lg, body = ops.LearnGraphs("X.learn()"), Body()
    assert [lg.run("k", body, eligible=False) for _ in range(3)] == [False] * 3
    assert body.runs == 3 and fake["captures"] == 0 and not lg.graphs and lg.last is None
    assert "k" in lg.warm
    assert lg.run("k", body) is True, "the ineligible calls warmed the key: the first eligible call captures"


def test_ineligible_call_of_a_captured_key_runs_eagerly(fake):
    lg, a, b = ops.LearnGraphs("X.learn()"), Body(), Body()
    for _ in range(2):
        lg.run("a", a, warm_key="w")
        lg.run("b", b, warm_key="w")
    assert set(lg.graphs) == {"a", "b"} and replays() == 3
    runs = a.runs
    assert lg.run("a", a, eligible=False, warm_key="w") is False
    assert a.runs == runs + 1 and replays() == 3 and set(lg.graphs) == {"a", "b"} and not lg.failed
    assert lg.run("b", b, warm_key="w") is True and lg.run("a", a, warm_key="w") is True
    assert replays() == 5 and fake["captures"] == 2


def test_profiling_the_library_vetoes_capture_and_replay(fake, monkeypatch):
    lg, body = ops.LearnGraphs("X.learn()"), Body()
    lg.run("k", body)
    lg.run("k", body)
    monkeypatch.setitem(ops._PROF, "lib", True)
    assert lg.run("k", body) is False and replays() == 1 and body.runs == 3
    assert lg.run("other", body, warm_key="k") is False and fake["captures"] == 1


def test_failed_capture_falls_back_for_good(fake, capsys):
    lg, a, b = ops.LearnGraphs("TD3.learn()"), Body(), Body()
    lg.run("a", a, warm_key="w")
    assert lg.run("a", a, warm_key="w") is True
    fake["raise"][2] = RuntimeError("operation not permitted when stream is capturing")
    assert lg.run("b", b, warm_key="w") is False
    assert b.runs == 1, "the body still ran eagerly in the call whose capture failed"
    assert lg.failed and not lg.graphs and lg.last is None
    before = replays()
    for _ in range(3):
        assert lg.run("a", a, warm_key="w") is False and lg.run("b", b, warm_key="w") is False
    assert replays() == before, "no captured graph is replayed after a failure"
    assert fake["captures"] == 2 and a.runs == 2 + 3 and b.runs == 1 + 3
    out = capsys.readouterr().out
    assert out.count("running eagerly") == 1
    assert "[jorldy_amd] hipGraph capture of TD3.learn() failed (RuntimeError: operation not permitted when stream is capturing); running eagerly" in out


def test_keyboard_interrupt_propagates(fake):
    lg, body = ops.LearnGraphs("X.learn()"), Body()
    lg.run("k", body)
    fake["raise"][1] = KeyboardInterrupt()
    with pytest.raises(KeyboardInterrupt):
        lg.run("k", body)
    assert not lg.failed and not lg.graphs


def test_reset_drops_graphs_keeps_warm(fake):
    lg, body = ops.LearnGraphs("X.learn()"), Body()
    lg.run("k", body)
    lg.run("k", body)
    assert lg.graphs and lg.last is not None
    lg.reset()
    assert not lg.graphs and lg.last is None and lg.warm == {"k"} and not lg.failed
    assert lg.run("k", body) is True and fake["captures"] == 2, "still warm: the next eligible call captures at once"


def ppo_call(lg, key, pre, main, eligible=True, capture=True):
    """The split form of PPO._learn_launch: the key's pre-phase graph and the shared "main" graph around the host's shuffles."""
    if lg.ready(key, {key: pre, "main": main}, eligible, warm_key=key, capture=capture):
        lg.replay(key)
        lg.replay("main")
        return True
    pre()
    main()
    lg.warm.add(key)
    return False


def test_pair_captured_under_one_latch(fake):
    lg, pre, main = ops.LearnGraphs("learn()"), Body(), Body()
    k0, k1 = ("split", False), ("split", True)
    assert ppo_call(lg, k0, pre, main) is False
    assert ppo_call(lg, k0, pre, main, capture=False) is False, "capture held off: eager, nothing captured"
    assert fake["captures"] == 0
    assert ppo_call(lg, k0, pre, main) is True
    assert set(lg.graphs) == {k0, "main"} and fake["captures"] == 2 and lg.last is lg.graphs["main"]
    assert ppo_call(lg, k0, pre, main, capture=False) is True, "capture held off: what is held is still replayed"
    assert ppo_call(lg, k1, pre, main) is False, "an unseen key is eager for both halves"
    assert lg.graphs["main"].replays == 2
    assert ppo_call(lg, k1, pre, main) is True
    assert set(lg.graphs) == {k0, k1, "main"} and fake["captures"] == 3, '"main" is shared, not captured again'


def test_pair_failure_in_the_second_drops_the_first(fake, capsys):
    lg, pre, main = ops.LearnGraphs("learn()"), Body(), Body()
    key = ("split", False)
    ppo_call(lg, key, pre, main)
    fake["raise"][2] = RuntimeError("collective refused capture")
    assert ppo_call(lg, key, pre, main) is False
    assert fake["captures"] == 2 and len(FakeGraph.made) == 2, "the pre-phase graph was captured, then dropped with the failure"
    assert not lg.graphs and lg.failed and replays() == 0
    assert (pre.runs, main.runs) == (3, 2), "eager, captured pre-phase, eager again / eager twice"
    assert ppo_call(lg, key, pre, main) is False and fake["captures"] == 2
    assert capsys.readouterr().out.count("running eagerly") == 1
