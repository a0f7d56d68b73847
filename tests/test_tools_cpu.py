"""The suite's own instruments, checked on the CPU: the margin ledger (tests/margins.py), its merge tool (tools/margins_merge.py), the
float64 criterion (tests/fp64_truth.py) -- an optimizer step with a wrong bias correction must FAIL it, a correct one pass -- and the
Hopper CPU reference bench.py reports beside its `hopper` leg."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fp64_truth as T
import margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_margin_ledger_records_ratios_and_the_merge_flags_what_matters(tmp_path):
    margins.leq(2.0, 8.0, "a quarter")
    np.testing.assert_allclose(np.array([1.0, 2.0]), np.array([1.0, 2.0 + 3e-6]), rtol=0, atol=1e-5)  # wrapped by conftest: 0.3
    with pytest.raises(AssertionError):
        margins.leq(3.0, 2.0, "over")
    node = margins._node()
    ratios = sorted(round(r[0], 3) for r in margins._LEDGER[node])
    assert ratios == [0.25, 0.3, 1.5]
    margins._LEDGER.pop(node, None)  # a deliberate 1.5 must not show up in a dumped ledger
    # two boxes' ledgers: one test identical on both and below 0.5, one above 0.5 and different between the boxes
    boxes = []
    for i, hair in enumerate((0.62, 0.91)):
        p = tmp_path / f"box{i}.json"
        json.dump({"host": f"h{i}", "gpu": {"uuid": str(i)}, "n_tests": 2, "max_ratio": hair,
                   "tests": {"t::calm": {"worst_ratio": 0.2, "what": "x"}, "t::hair": {"worst_ratio": hair, "what": "y"}}}, open(p, "w"))
        boxes.append(str(p))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "margins_merge.py")] + boxes, capture_output=True, text=True, check=True)
    m = json.loads(out.stdout)
    assert m["max_ratio"] == 0.91 and [r["test"] for r in m["over_half"]] == ["t::hair"] and m["over_half_and_box_dependent"] == ["t::hair"]
    calm = [r for r in m["tests"] if r["test"] == "t::calm"][0]
    assert calm["same_on_every_box"] and calm["worst_ratio"] == 0.2


def _tiny():
    torch.manual_seed(0)
    m64 = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ReLU(), torch.nn.Linear(8, 3)).double()
    T.round_to_fp32_(m64)
    return m64, T.as32(m64)


def test_float64_criterion_passes_fp32_arithmetic_and_rejects_a_wrong_bias_correction():
    """check_first_step_from_our_gradient: float64 Adam fed "our" gradient must land on "our" weights.  "Ours" here is an fp32 Adam
    step done by hand -- once correctly (passes), once with the bias corrections of step 2 instead of step 1 (a quarter of a step), and
    once with the update simply 5 % too long (what VERDICT r3 weak #12 said no test would notice) -- both must fail."""
    m64, m32 = _tiny()
    x = torch.randn(16, 6)
    loss = (m32(x) ** 2).mean()
    loss.backward()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    w0 = {k: v.detach().clone() for k, v in m32.state_dict().items()}
    g = {k: p.grad.detach().clone() for k, p in m32.named_parameters()}

    def adam_fp32(step_for_bc):
        out = {}
        for k in w0:
            m = (1 - b1) * g[k]
            v = (1 - b2) * g[k] * g[k]
            bc1, bc2 = 1 - b1 ** step_for_bc, 1 - b2 ** step_for_bc
            out[k] = w0[k] - (lr / bc1) * (m / (v.sqrt() / (bc2 ** 0.5) + eps))
        return out

    make = lambda ps: torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps)
    T.check_first_step_from_our_gradient(w0, g, adam_fp32(1), make, lr, "correct step")
    with pytest.raises(AssertionError):
        T.check_first_step_from_our_gradient(w0, g, adam_fp32(2), make, lr, "bias correction of the wrong step")
    good = adam_fp32(1)
    with pytest.raises(AssertionError):
        T.check_first_step_from_our_gradient(w0, g, {k: w0[k] + 1.05 * (good[k] - w0[k]) for k in w0}, make, lr, "a step 5 % too long")


def test_vs_exact_allows_what_fp32_itself_cannot_do_better_and_nothing_more():
    exact = torch.linspace(-1, 1, 101, dtype=torch.float64)
    ref32 = exact + 3e-5          # the fp32 comparator is itself 3e-5 away: 6e-5 allowed
    T.vs_exact(exact + 5e-5, exact, ref32, 1e-5, "within twice the comparator's own error")
    with pytest.raises(AssertionError):
        T.vs_exact(exact + 7e-5, exact, ref32, 1e-5, "beyond it")
    with pytest.raises(AssertionError):
        T.vs_exact(exact + 2e-5, exact, exact.clone(), 1e-5, "comparator exact: only the tolerance is left")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(b)
    finally:
        sys.argv = argv
    return b


def test_hopper_cpu_reference_runs_the_ports_learner_at_the_legs_shapes():
    b = _bench()
    threads = torch.get_num_threads()
    try:
        r = b.hopper_cpu_reference(W=2, T=64, B=32, epochs=2)
    finally:
        torch.set_num_threads(threads)
    assert r["kind"] == "port" and r["unit"] == "transitions/s" and r["value"] > 0 and abs(r["value"] * r["s_per_learn"] - 128) < 1e-6 * 128
    assert "2 epochs x 4 minibatches of 32" in r["sample"]


def test_bench_plain_run_leaves_every_other_measurement_to_full():
    b = _bench()
    plain = b.parse(["--steps", "7", "--warmup", "2"])
    assert plain.steps == 7 and plain.warmup == 2 and not plain.full and plain.dump_outputs is None
    assert all(getattr(plain, k) for k in b.FULL_ONLY)
    full = b.parse(["--full", "--no-dqn", "--dump-outputs", "out"])
    assert full.full and full.no_dqn and full.dump_outputs == "out" and not any(getattr(full, k) for k in b.FULL_ONLY if k != "no_dqn")
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            b.parse(bad)


def test_bench_dump_writes_float_arrays_within_the_budget(tmp_path):
    b = _bench()
    arrays = {"rollout_state": np.arange(12, dtype=np.float32).reshape(3, 4), "result_loss": np.float64(0.25)}
    b.write_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["result_loss.npy", "rollout_state.npy"]
    back = np.load(tmp_path / "d" / "rollout_state.npy")
    assert back.dtype == np.float32 and np.array_equal(back, arrays["rollout_state"]) and float(np.load(tmp_path / "d" / "result_loss.npy")) == 0.25
    with pytest.raises(ValueError):
        b.write_outputs(str(tmp_path / "e"), {"action": np.zeros(3, np.int64)})
    with pytest.raises(ValueError):
        b.write_outputs(str(tmp_path / "f"), {"big": np.zeros(b.DUMP_MAX_BYTES // 8 + 1, np.float64)})
    assert not os.path.exists(tmp_path / "e") and not os.path.exists(tmp_path / "f")


def test_bench_dump_thins_a_rollout_over_the_budget_to_a_seeded_sample(monkeypatch):
    """last_step_outputs on a stand-in agent (host tensors): the whole rollout when it fits, the same fixed sample of rows on every call when not."""
    from types import SimpleNamespace

    b = _bench()
    cols = {"state": torch.arange(400.0).reshape(100, 4), "action": torch.arange(100, dtype=torch.int64).reshape(100, 1), "done": torch.ones(100, 1, dtype=torch.uint8)}
    store = SimpleNamespace(names=list(cols), device=torch.device("cpu"), column=cols.__getitem__)
    agent = SimpleNamespace(memory=SimpleNamespace(_store=store), network=torch.nn.Linear(3, 2))
    whole = b.last_step_outputs(agent, 60)
    assert np.array_equal(whole["rollout_state"], cols["state"][:60].numpy()) and whole["rollout_action"].dtype == np.float32
    assert whole["network_weight"].shape == (2, 3) and whole["rollout_done"].shape == (60, 1)
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 2 * (32 + 40 * 24))  # the network's 32 bytes + 40 rows of 24 bytes, in half the budget
    a, c = b.last_step_outputs(agent, 60), b.last_step_outputs(agent, 60)
    rows = a["rollout_action"][:, 0].astype(int)
    assert len(rows) == 40 and np.all(np.diff(rows) > 0) and rows.max() < 60 and np.array_equal(a["rollout_state"], c["rollout_state"])
    assert np.array_equal(a["rollout_state"], cols["state"].numpy()[rows])


# ---------------------------------------------------------------------------------- oracle/refkit.py, the fixture generators' toolkit
def _fake_reference(tmp_path):
    ref = tmp_path / "checkout"
    (ref / "jorldy" / "core" / "env" / "mlagents").mkdir(parents=True)
    (ref / "jorldy" / "core" / "__pycache__").mkdir()
    (ref / "jorldy" / "core" / "__init__.py").write_text("")
    (ref / "jorldy" / "core" / "__pycache__" / "stale.pyc").write_bytes(b"\0")
    (ref / "jorldy" / "core" / "env" / "mlagents" / "x.bin").write_bytes(b"\0" * 16)
    (ref / "jorldy" / "refkit_probe.py").write_text("import core\nWHERE = __file__\nCORE = core.__file__\n")
    return str(ref)


def _check_inside_the_copy(copy):
    import refkit_probe

    assert os.path.samefile(os.getcwd(), copy) and sys.path[0] == copy and sys.dont_write_bytecode
    assert os.path.samefile(refkit_probe.WHERE, os.path.join(copy, "refkit_probe.py")) and os.path.samefile(refkit_probe.CORE, os.path.join(copy, "core", "__init__.py"))
    assert os.path.isdir(os.path.join(copy, "core", "env")) and not os.path.exists(os.path.join(copy, "core", "env", "mlagents"))
    assert not [d for d, sub, _ in os.walk(copy) if "__pycache__" in sub]


def test_staged_reference_imports_from_a_scratch_copy_and_undoes_itself_also_on_an_exception(tmp_path):
    from oracle import refkit

    ref = _fake_reference(tmp_path)
    before = (os.getcwd(), list(sys.path), sys.dont_write_bytecode)
    with refkit.staged_reference(ref) as copy:
        _check_inside_the_copy(copy)
    assert (os.getcwd(), sys.path, sys.dont_write_bytecode) == before and not os.path.exists(os.path.dirname(copy))
    assert "refkit_probe" not in sys.modules and "core" not in sys.modules
    seen = []
    with pytest.raises(RuntimeError):
        with refkit.staged_reference(ref) as copy2:
            seen.append(copy2)
            _check_inside_the_copy(copy2)  # imported afresh, from the second copy
            raise RuntimeError("inside the block")
    assert seen[0] != copy and (os.getcwd(), sys.path, sys.dont_write_bytecode) == before and not os.path.exists(os.path.dirname(seen[0]))
    assert "refkit_probe" not in sys.modules and os.path.exists(os.path.join(ref, "jorldy", "core", "env", "mlagents", "x.bin"))


def test_line_tap_snapshots_named_locals_in_front_of_the_marked_line():
    from oracle import refkit

    def three_lines(x):
        a = x + 1
        b = a * 2  # the marked line
        return b

    tracer = sys.gettrace()
    try:
        tap = refkit.LineTap(three_lines, {"m": ("# the marked line", ["x", "a", "b", "absent"])})
        calls = []
        tap.on_line["m"] = lambda frame: calls.append(sorted(frame.f_locals))
        with tap:
            assert three_lines(3) == 8 and three_lines(5) == 12
        assert sys.gettrace() is None
        assert calls == [["a", "x"], ["a", "x"]], "on_line runs in front of the marked line: b is not bound yet"
        assert [sorted(r) for r in tap.records["m"]] == [["a", "x"], ["a", "x"]] and [int(r["a"]) for r in tap.records["m"]] == [4, 6]
        assert isinstance(tap.records["m"][0]["x"], np.ndarray)
        with pytest.raises(AssertionError, match="not found"):
            refkit.LineTap(three_lines, {"m": ("a line this function does not have", [])})
    finally:
        sys.settrace(tracer)


def test_keeper_is_the_identity_at_zero_and_synths_thin_above():
    from oracle import refkit, synth

    big, small = np.arange(20000, dtype=np.float32).reshape(100, 200), np.arange(12.0)
    assert refkit.keeper(0)(big) is big
    for limit in (100, 8192):
        assert np.array_equal(refkit.keeper(limit)(big), synth.thin(big, limit)) and refkit.keeper(limit)(big).size < big.size
        assert np.array_equal(refkit.keeper(limit)(small), small)
