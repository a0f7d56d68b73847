"""What every fixture generator shares: staging the reference, the generator main, the line tap, weights, storage layouts and curve loops.

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists); nothing on a GPU machine runs this or reads the
reference.  oracle/gen_golden.py, the tools/gen_golden_<agent>.py files and the two other oracle/ scripts that run the UNMODIFIED reference keep
what is theirs alone -- specs, tapped names and marker substrings, agent keyword arguments, agent-specific recording, assertions -- and take
the rest from here.  This file holds none of the reference's text: the marker substrings a tap looks for are passed in by its caller.

  staged_reference(ref)   scratch copy of <ref>/jorldy, imported from there; undone on exit
  run(...)                the generator main: --ref --out --only [--threads]
  LineTap                 snapshot named locals of a function in front of marked source lines
  seed_rngs, grads_of, grad_norm, retaining_hooks, last_outputs, multiplier_state, multiplier_grads
  set_weights, fill_transitions, dump_buffer, dump_rollout, keeper, put_hyper, save_fixture
  value_agent, record_value_learn, store_step, put_result   the value family (one network, one target, one optimizer)
  actor_critic_agent, store_actor_critic_record          the actor-critic family (several networks and optimizers)
  value_cartpole_curve, control_curve, sync_cartpole_curve, seeded_curves, curve_doc, write_curves
"""
import argparse
import contextlib
import inspect
import json
import os
import shutil
import sys
import tempfile

import numpy as np

from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE_SEED = 20260925
FILL_SEED = 17


# ---------------------------------------------------------------------------------- staging and the generator main
def _skip(directory, names):
    """No Unity binaries (core/env/mlagents) and no bytecode in the scratch copy."""
    drop = {"__pycache__"}
    if os.path.basename(directory) == "env" and os.path.basename(os.path.dirname(directory)) == "core":
        drop.add("mlagents")
    return drop & set(names)


@contextlib.contextmanager
def staged_reference(ref):
    """Import the reference from a scratch copy of <ref>/jorldy: importing `core` rewrites its `_*_dict.txt` files, and the checkout stays as
    it is.  Inside the block the copy is the working directory and first on sys.path, and no bytecode is written.  On exit, an exception
    included, the working directory, sys.path and the bytecode switch are what they were, the modules loaded from the copy are forgotten and
    the copy is removed."""
    scratch = tempfile.mkdtemp(prefix="jref_")
    cwd, path, bytecode = os.getcwd(), list(sys.path), sys.dont_write_bytecode
    try:
        copy = shutil.copytree(os.path.join(ref, "jorldy"), os.path.join(scratch, "jorldy"), symlinks=True, ignore=_skip)
        sys.dont_write_bytecode = True
        os.chdir(copy)
        sys.path.insert(0, copy)
        yield copy
    finally:
        os.chdir(cwd)
        sys.path[:] = path
        sys.dont_write_bytecode = bytecode
        for name, mod in list(sys.modules.items()):
            if (getattr(mod, "__file__", None) or "").startswith(scratch + os.sep):
                del sys.modules[name]
        shutil.rmtree(scratch, ignore_errors=True)


def each(gen_fixture, names):
    """The usual fixture half of a generator: gen_fixture(name, out_dir) for every name, behind the word `fixtures` of --only."""
    return {"fixtures": lambda out_dir: [gen_fixture(name, out_dir) for name in names]}


def run(fixtures, curves=None, threads=None, ref=None, default=None, description=None):
    """The main of a generator.  `fixtures`: {word of --only: callable(out_dir)}, run in that order with ONE torch thread (deterministic
    reductions); `curves`: callable(out_dir, threads) behind the word `curves`, run with --threads (default `threads`) torch threads.
    `ref`: the default of --ref (required when None); `default`: the words of a plain run (every word when None)."""
    words = list(fixtures) + (["curves"] if curves else [])
    default = default or ",".join(words)
    ap = argparse.ArgumentParser(description=description)
    if ref is None:
        ap.add_argument("--ref", required=True, help="checkout of the reference (the directory that holds jorldy/)")
    else:
        ap.add_argument("--ref", default=ref)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--only", default=default, help="comma-separated, of: " + " ".join(words))
    if curves:
        ap.add_argument("--threads", type=int, default=threads, help="torch threads of the curve runs (the fixtures always use one)")
    args = ap.parse_args()
    todo = (args.only or default).split(",")
    unknown = [w for w in todo if w not in words]
    if unknown:
        ap.error(f"--only: unknown {unknown}; known: {' '.join(words)}")
    out_dir = os.path.abspath(args.out)
    os.makedirs(out_dir, exist_ok=True)
    with staged_reference(args.ref):
        import torch

        torch.set_num_threads(1)
        for word, gen in fixtures.items():
            if word in todo:
                gen(out_dir)
        if "curves" in todo:
            torch.set_num_threads(args.threads)
            curves(out_dir, args.threads)
    print("written to", out_dir)


# ---------------------------------------------------------------------------------- the tap and small helpers
def _to_np(v):
    import torch

    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy().copy()
    if isinstance(v, np.ndarray):
        return v.copy()
    if isinstance(v, (list, tuple)) and v and isinstance(v[0], (int, float, np.integer, np.floating)):
        return np.asarray(v)
    if isinstance(v, (int, float, bool, np.integer, np.floating)):
        return np.asarray(v)
    return None


class LineTap:
    """Snapshot named locals of `func` each time execution reaches a source line
    containing one of the given marker substrings (BEFORE that line executes),
    and once more at return (key '<return>')."""

    def __init__(self, func, markers):
        self.code = func.__code__
        src, first = inspect.getsourcelines(func)
        self.line_to_key = {}
        for key, (needle, names) in markers.items():
            hits = [i for i, s in enumerate(src) if needle in s]
            assert hits, f"marker {needle!r} not found in {func.__qualname__}"
            self.line_to_key[first + hits[0]] = (key, names)
        self.ret_names = markers.get("<return>", (None, ()))[1] if "<return>" in markers else ()
        self.records = {}  # key -> list of dict
        self.on_line = {}  # key -> callback(frame)

    def _local(self, frame, event, arg):
        if event == "line" and frame.f_lineno in self.line_to_key:
            key, names = self.line_to_key[frame.f_lineno]
            if key in self.on_line:
                self.on_line[key](frame)
            snap = {}
            for n in names:
                if n in frame.f_locals:
                    a = _to_np(frame.f_locals[n])
                    if a is not None:
                        snap[n] = a
            self.records.setdefault(key, []).append(snap)
        return self._local

    def _global(self, frame, event, arg):
        if event == "call" and frame.f_code is self.code:
            return self._local
        return None

    def __enter__(self):
        sys.settrace(self._global)
        return self

    def __exit__(self, *a):
        sys.settrace(None)


def flat(prefix, d, out):
    for k, v in d.items():
        out[f"{prefix}{k}"] = v


def sd_to_np(sd):
    return {k: v.detach().cpu().numpy().copy() for k, v in sd.items()}


def grads_of(module, trainable_only=False):
    return {k: p.grad.detach().numpy().copy() for k, p in module.named_parameters() if p.requires_grad or not trainable_only}


def grad_norm(grads):
    return np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in grads.values()))


def seed_rngs(seed):
    import torch

    np.random.seed(seed)
    torch.manual_seed(seed)


def retaining_hooks(mods):
    """{tag: module} -> ({tag: [every forward output, its gradient retained]}, the hook handles)."""
    outs = {}

    def mk_hook(tag):
        def hook(mod, inp, outp):
            if outp.requires_grad:
                outp.retain_grad()
            outs.setdefault(tag, []).append(outp)

        return hook

    return outs, [mod.register_forward_hook(mk_hook(tag)) for tag, mod in mods.items()]


def last_outputs(outs):
    """Of retaining_hooks' lists: {tag: the last output, d_<tag>: its gradient}."""
    out = {}
    for tag, lst in outs.items():
        out[tag] = lst[-1].detach().numpy().copy()
        out["d_" + tag] = lst[-1].grad.detach().numpy().copy()
    return out


def multiplier_state(agent, names, optimizer):
    """The learned scalar multipliers `names` of an agent with their Adam moments in `optimizer` (zeros before the first step)."""
    out = {}
    for k in names:
        p = getattr(agent, k)
        st = optimizer.state.get(p)
        out[k] = np.asarray(float(p.detach()), np.float32)
        out[k + "/has_state"] = np.asarray(int(bool(st)))
        out[k + "/exp_avg"] = np.asarray(float(st["exp_avg"]) if st else 0.0, np.float32)
        out[k + "/exp_avg_sq"] = np.asarray(float(st["exp_avg_sq"]) if st else 0.0, np.float32)
        out[k + "/step"] = np.asarray(int(float(st["step"])) if st else 0)
    return out


def multiplier_grads(agent, names):
    """NaN and has_grad = 0 where the reference's loss gives a multiplier no gradient."""
    out = {k: np.asarray(float(getattr(agent, k).grad) if getattr(agent, k).grad is not None else np.nan, np.float32) for k in names}
    out.update({k + "/has_grad": np.asarray(int(getattr(agent, k).grad is not None)) for k in names})
    return out


# ---------------------------------------------------------------------------------- weights, inputs and storage
def set_weights(modules, recipe, seed0, perturb):
    """Starting weights that do not depend on torch's initialisers.  `recipe` (synth.recipe_state_dict, synth.ppo_recipe) given: module i gets
    recipe(its shapes, seed0 + i), regenerated from the seed by the reader.  None: p += perturb * randn_like(p), module after module --
    independent draws, so every target differs from its online net."""
    import torch

    with torch.no_grad():
        for i, mod in enumerate(modules):
            if recipe:
                rec = recipe({k: tuple(v.shape) for k, v in mod.state_dict().items()}, seed0 + i)
                for k, p in mod.named_parameters():
                    p.copy_(torch.from_numpy(rec[k]))
            else:
                for p in mod.parameters():
                    p.add_(perturb * torch.randn_like(p))


def _fill(agent, n, S, A, rng, n_step=None, with_q=False):
    """Drive interact_callback + memory.store the way Actor.run / run_mode do."""
    for i in range(n):
        t = synth.raw_transition(rng, S, A, with_q)
        t = agent.interact_callback(t)
        if t:
            agent.memory.store([t])


def fill_transitions(n, S, A, seed):
    """n synthetic continuous-control transitions (also what the tests store into the HIP agent's buffer: the fixture keeps them as buf_*)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        out.append({"state": rng.randn(1, S).astype(np.float32), "action": np.tanh(rng.randn(1, A)).astype(np.float32),
                    "reward": rng.choice([-1.0, 0.0, 1.0, 0.5], size=(1, 1)), "next_state": rng.randn(1, S).astype(np.float32),
                    "done": np.asarray([[rng.rand() < 0.1]])})
    return out


def dump_buffer(agent, out):
    """The replay columns in slot order as buf_*, so that a reader can load its own buffer identically."""
    n = agent.memory.size
    for k in agent.memory.buffer[0].keys():
        out[f"buf_{k}"] = np.concatenate([agent.memory.buffer[i][k] for i in range(n)], 0)


def dump_rollout(out, prefix, trs, recipe):
    """A rollout of synth's: in full, or (recipe: the reader regenerates it from its seed) as checksums of 64 of its rows."""
    M = len(trs)
    if recipe:
        for k in ("state", "reward", "action"):
            out[f"{prefix}in_{k}_check"] = synth.row_checksum(np.concatenate([t[k] for t in trs], 0).astype(np.float32))[:: max(1, M // 64)]
    else:
        for k in ("state", "next_state", "reward", "done", "action"):
            out[f"{prefix}in_{k}"] = np.concatenate([t[k] for t in trs], 0)


def keeper(limit):
    """hyper/thin_limit: 0 keeps every array whole, n stores arrays larger than n as synth.thin(v, n) samples."""
    return (lambda v: synth.thin(v, limit)) if limit else (lambda v: v)


def put_hyper(out, hyper):
    for k, v in hyper.items():
        out[f"hyper/{k}"] = np.asarray(v)


def save_fixture(out_dir, name, out, cap=None, note=""):
    path = os.path.join(out_dir, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(name, f"{size} bytes", note)
    assert cap is None or size <= cap, f"{path}: {size} bytes, more than the {cap} this family allows itself"


# ---------------------------------------------------------------------------------- the value family
def value_agent(cls, kw, recipe, fill=200):
    """The value family's starting point: the agent under seed 3, recipe (seed, seed + 1) or perturbed weights for online and target,
    `fill` synthetic env steps of RandomState(FILL_SEED) -> (agent, out) with the replay columns in `out`."""
    seed_rngs(3)
    agent = cls(**kw)
    set_weights([agent.network, agent.target_network], synth.recipe_state_dict if recipe else None, RECIPE_SEED, 0.1)
    agent.memory.first_store = False
    _fill(agent, fill, kw["state_size"], kw["action_size"], np.random.RandomState(FILL_SEED))
    out = {}
    dump_buffer(agent, out)
    return agent, out


def store_step(out, agent, grads, sd0, sdt, thin=None, moments=(), norm=True, sd0_min=0):
    """Gradient, weights before (online, target) and after, and the optimizer moments `moments` after one step.  thin None: every tensor in
    full under grad/ sd0/ sdt/ sd1/ opt1/.  thin given (recipe fixtures): samples under *_thin/, the gradient's norm (`norm`) and largest
    entry per tensor beside them; of the starting weights, which the reader regenerates, only tensors over sd0_min entries."""
    sd1 = sd_to_np(agent.network.state_dict())
    moments = {m: {k: agent.optimizer.state[p][m].detach().numpy().copy() for k, p in agent.network.named_parameters()} for m in moments}
    if thin:
        flat("grad_thin/", {k: thin(v) for k, v in grads.items()}, out)
        if norm:
            out["grad_norm"] = grad_norm(grads)
        for k, v in grads.items():
            out[f"grad_absmax/{k}"] = np.abs(v).max()
        flat("sd0_thin/", {k: thin(v) for k, v in sd0.items() if v.size > sd0_min}, out)
        flat("sdt_thin/", {k: thin(v) for k, v in sdt.items() if v.size > sd0_min}, out)
        flat("sd1_thin/", {k: thin(v) for k, v in sd1.items()}, out)
    else:
        flat("grad/", grads, out)
        flat("sd0/", sd0, out)
        flat("sdt/", sdt, out)
        flat("sd1/", sd1, out)
    for m, d in moments.items():
        flat(f"opt1_thin/{m}/" if thin else f"opt1/{m}/", {k: thin(v) if thin else v for k, v in d.items()}, out)


def record_value_learn(agent, markers, out, watch=None, at="pre_step", name="q_all", extra=None, around=None, rename=None, first=None):
    """One learn() of the reference agent under the line tap (seeds 42), written to `out`: what `first()` returns, learn/* (the locals
    `markers["pre_step"]` names, `rename`d where asked), learn/<name> and learn/d_<name>.  -> ((gradients, online and target weights before:
    what store_step takes next), learn()'s result for put_result); what a fixture stores in between is its generator's.
    <name> is the tensor whose gradient is retained, taken in front of the line of marker `at`: the local called `watch`, or (watch None) the
    output of network(state) -- an unnamed temporary inside learn(), which a forward hook keeps; the network then runs forward exactly once.
    `extra(frame)` -> further learn/ entries computed at that line; `around`: a context manager held over the learn()."""
    sd0, sdt = sd_to_np(agent.network.state_dict()), sd_to_np(agent.target_network.state_dict())
    tap = LineTap(type(agent).learn, markers)
    grads, head, forwards, kept = {}, {}, [], []
    hook = agent.network.register_forward_hook(lambda mod, inp, outp: forwards.append(outp)) if watch is None else None

    def on_at(frame):
        kept.append(forwards[-1] if watch is None else frame.f_locals[watch])
        kept[0].retain_grad()
        head[name] = kept[0].detach().numpy().copy()
        if extra:
            head.update(extra(frame))

    def on_step(frame):
        grads.update(grads_of(agent.network))
        head["d_" + name] = kept[0].grad.detach().numpy().copy()

    tap.on_line[at], tap.on_line["step"] = on_at, on_step
    seed_rngs(42)
    with around or contextlib.nullcontext(), tap:
        result = agent.learn()
    if hook:
        hook.remove()
    assert len(kept) == 1 and (watch is not None or len(forwards) == 1)
    out.update(first() if first else {})
    rec = dict(tap.records["pre_step"][0])
    for local, key in (rename or {}).items():
        rec[key] = rec.pop(local)
    flat("learn/", rec, out)
    flat("learn/", head, out)
    return (grads, sd0, sdt), result


def put_result(out, result):
    for k, v in result.items():
        out[f"result/{k}"] = np.asarray(v)
    print({k: float(v) for k, v in result.items()})


# ---------------------------------------------------------------------------------- the actor-critic family
def actor_critic_agent(cls, kw, nets, out, recipe, perturb, limit, init_seed, fill, tweak=None):
    """The actor-critic family's starting point, written to `out`: init_thin/ (the initial weights of a fresh agent under init_seed:
    construction order, initialiser gains), then the fixture's own agent (seed 3) with recipe (seed + position in `nets`) or perturbed
    weights, `tweak(agent)`ed, its buffer holding `fill` fill_transitions (buf_*), and sd0/ its starting weights -- in full unless they come
    from the recipe.  -> (agent, {net: starting weights}, keeper(limit))"""
    import torch

    torch.manual_seed(init_seed)
    fresh = cls(**kw)
    for net in nets:
        flat(f"init_thin/{net}/", {k: synth.thin(v) for k, v in sd_to_np(getattr(fresh, net).state_dict()).items()}, out)
    seed_rngs(3)
    agent = cls(**kw)
    set_weights([getattr(agent, net) for net in nets], synth.recipe_state_dict if recipe else None, RECIPE_SEED, perturb)
    if tweak:
        with torch.no_grad():
            tweak(agent)
    agent.memory.first_store = False
    agent.memory.store(fill_transitions(fill, kw["state_size"], kw["action_size"], FILL_SEED))
    dump_buffer(agent, out)
    keep = keeper(limit)
    sd0 = {net: sd_to_np(getattr(agent, net).state_dict()) for net in nets}
    for net in nets:
        flat(f"sd0/{net}/", {k: keep(v) if recipe else v for k, v in sd0[net].items()}, out)
    return agent, sd0, keep


def store_actor_critic_record(out, r, agent, nets, opts, start, rec, grads, result, keep, then=None):
    """Record r<r>/ of one learn(): learn/ and result/, `then` (further entries of the record), the gradients with their largest entries, per network either `unchanged` = 1 (learn()
    left it bit-identical to `start`) or its end weights, and the Adam moments of `opts` = ((net, optimizer attribute), ...)."""
    flat(f"r{r}/learn/", rec, out)
    flat(f"r{r}/result/", result, out)
    flat(f"r{r}/", then or {}, out)
    flat(f"r{r}/grad/", {k: keep(v) for k, v in grads.items()}, out)
    for k, v in grads.items():
        out[f"r{r}/grad_absmax/{k}"] = np.abs(v).max()
    for net in nets:
        sd1 = sd_to_np(getattr(agent, net).state_dict())
        same = all(np.array_equal(sd1[k], start[net][k]) for k in sd1)
        out[f"r{r}/unchanged/{net}"] = np.asarray(int(same))
        if not same:
            flat(f"r{r}/sd1/{net}/", {k: keep(v) for k, v in sd1.items()}, out)
    for net, oname in opts:
        for k, p in getattr(agent, net).named_parameters():
            st = getattr(agent, oname).state.get(p)
            if st:
                out[f"r{r}/opt/{net}/exp_avg/{k}"] = keep(st["exp_avg"].detach().numpy().copy())
                out[f"r{r}/opt/{net}/exp_avg_sq/{k}"] = keep(st["exp_avg_sq"].detach().numpy().copy())


# ---------------------------------------------------------------------------------- curves
def value_cartpole_curve(agent, seed, steps, chunk):
    """The single-mode loop of tests/test_learning_curve_gpu.py::_dqn_curve (act, step, process([transition], step)) with a reference agent
    on the oracle's CartPole -> mean episode length per `chunk` env steps."""
    from oracle.dqn_port import make_env

    env, state = make_env(1000 + seed)
    out, lens, ep = [], [], 0
    for step in range(1, steps + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"]).reshape(-1))
        tr = {"state": state, "next_state": nxt.astype(np.float32), "reward": rew.reshape(1, 1).astype(np.float64), "done": done.reshape(1, 1)}
        tr.update(a)
        agent.process([tr], step)
        state = env.obs().astype(np.float32)
        ep += 1
        if bool(done.reshape(-1)[0]):
            lens.append(ep)
            ep = 0
        if step % chunk == 0:
            out.append(float(np.mean(lens)) if lens else float(ep))
            lens = []
    return out


def control_curve(agent, env, steps, chunk):
    """The single-mode loop (act, step, process([transition], step)) -> mean reward per `chunk` env steps."""
    out, acc = [], []
    state = env.obs()
    for step in range(1, steps + 1):
        a = agent.act(state, True)
        nxt, rew, done = env.step(np.asarray(a["action"], dtype=np.float32).reshape(1, -1))
        tr = {"state": state, "next_state": np.asarray(nxt, dtype=np.float32), "reward": np.asarray(rew, dtype=np.float64).reshape(1, 1),
              "done": np.asarray(done).astype(bool).reshape(1, 1)}
        tr.update(a)
        agent.process([tr], step)
        state = env.obs()
        acc.append(float(np.asarray(rew).reshape(-1)[0]))
        if step % chunk == 0:
            out.append(float(np.mean(acc)))
            acc = []
    return out


def control_oracle_curve(agent, seed, c):
    """control_curve on the oracle's control env of c["S"] x c["A"] (seed 1000 + seed) for c["steps"] steps in chunks of c["chunk"]."""
    from oracle.jorldy_oracle import ControlOracle

    agent.memory.first_store = False
    return control_curve(agent, ControlOracle(1, c["S"], c["A"], seed=1000 + seed), c["steps"], c["chunk"])


def sync_cartpole_curve(agent, seed, workers, n_step, iterations, per_iter=None):
    """The synchronous on-policy loop (`workers` CartPoles of the oracle's, n_step steps each, one process() per iteration) -> mean episode
    length per iteration (transitions / episode ends).  per_iter(agent) runs after every process()."""
    from oracle import ppo_port as P

    envs = [P._OneEnv(seed=1000 * seed + w) for w in range(workers)]
    states = [e.reset_obs() for e in envs]
    curve, step = [], 0
    for _ in range(iterations):
        trs = P.sync_iteration(agent, envs, states, n_step)  # Actor.run of the distributed manager with agent.act of whoever is passed
        curve.append(len(trs) / max(1, sum(int(t["done"][0, 0]) for t in trs)))
        step += n_step
        agent.process(trs, step)
        if per_iter:
            per_iter(agent)
    return curve


def seeded_curves(curve, seeds, label, digits=1):
    """[curve(seed) for every seed], each printed as it ends."""
    curves = []
    for s in seeds:
        curves.append(curve(s))
        print(label, "curve seed", s, [round(v, digits) for v in curves[-1]], flush=True)
    return curves


def curve_doc(generator, seeds, threads, **rest):
    return {"generator": generator, "seeds": list(seeds), "torch_threads": threads, **rest}


def write_curves(path, doc, indent=1):
    with open(path, "w") as f:
        json.dump(doc, f, indent=indent)
