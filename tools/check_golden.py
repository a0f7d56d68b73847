#!/usr/bin/env python3
"""Do the fixture generators still reproduce the committed fixtures?  Nothing else keeps them honest: no test executes them.

TEST INFRASTRUCTURE ONLY, for the build machine (where a checkout of the reference exists), like the generators themselves; nothing under
tests/, bench.py or smoke() calls it.  Runs the fixture half of oracle/gen_golden.py and of every tools/gen_golden_<agent>.py, each in a process
of its own, into a temporary directory and compares every .npz written with tests/golden/: the same keys, per key the same dtype and shape,
and equal values (NaN equal to NaN: the V-MPO and MPO fixtures store NaN for a multiplier gradient the reference does not have).  With
--curves the named generators' curve halves run too, with the torch thread count their committed file records, and the JSON documents are
compared as parsed.  Lists every file and key that differs and exits 1 if there is one.

Usage:  python tools/check_golden.py --ref <reference checkout> [--curves td3,qrdqn,vmpo] [--against tests/golden] [--tools td3,sac,oracle]
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ("qrdqn", "mdqn", "iqn", "miqn", "riqn", "noisy", "td3", "sac", "vmpo", "mpo", "mpo_continuous", "icm", "r2d2", "reinforce", "rnd")


def npz_differences(new, old):
    """-> what differs between two .npz files, one line per key."""
    a, b = np.load(new), np.load(old)
    out = [f"key {k} only in the {'new' if k in a.files else 'committed'} file" for k in sorted(set(a.files) ^ set(b.files))]
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            out.append(f"key {k}: {x.dtype}{x.shape} new, {y.dtype}{y.shape} committed")
        elif not np.array_equal(x, y, equal_nan=x.dtype.kind in "fc"):
            out.append(f"key {k}: values differ")
    return out


def generate(script, ref, out_dir, words, threads=None):
    cmd = [sys.executable, os.path.join(ROOT, script), "--ref", ref, "--out", out_dir] + (["--only", words] if words else [])
    t0 = time.time()
    # a curve run takes minutes and prints every seed as it ends: that stays visible
    subprocess.run(cmd + (["--threads", str(threads)] if threads else []), check=True, stdout=None if threads else subprocess.DEVNULL)
    print(f"{script} {words or ''}: {time.time() - t0:.0f} s", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference (the directory that holds jorldy/)")
    ap.add_argument("--curves", default="", help="comma-separated generators whose curve file is regenerated and compared too, e.g. td3,qrdqn,vmpo")
    ap.add_argument("--against", default=os.path.join(ROOT, "tests", "golden"), help="the directory to compare with")
    ap.add_argument("--tools", default=",".join(TOOLS + ("oracle",)), help="the generators to run (oracle = oracle/gen_golden.py)")
    args = ap.parse_args()
    bad = []
    with tempfile.TemporaryDirectory(prefix="jgold_") as tmp:
        for tool in args.tools.split(","):
            if tool == "oracle":
                generate("oracle/gen_golden.py", args.ref, tmp, None)
            else:
                generate(f"tools/gen_golden_{tool}.py", args.ref, tmp, "fixtures")
        written = sorted(glob.glob(os.path.join(tmp, "*.npz")))
        for path in written:
            name = os.path.basename(path)
            old = os.path.join(args.against, name)
            bad += [f"{name}: {d}" for d in (npz_differences(path, old) if os.path.exists(old) else ["not in " + args.against])]
        print(f"{len(written)} .npz files compared with {args.against}", flush=True)
        for tool in filter(None, args.curves.split(",")):
            name = f"curves_reference_{'icm_ppo' if tool == 'icm' else tool}.json"
            with open(os.path.join(args.against, name)) as f:
                old = json.load(f)
            generate(f"tools/gen_golden_{tool}.py", args.ref, tmp, "curves", threads=old["torch_threads"])
            with open(os.path.join(tmp, name)) as f:
                new = json.load(f)
            bad += [f"{name}: key {k} differs" for k in sorted(set(new) | set(old)) if k not in new or k not in old or new[k] != old[k]]
    for line in bad:
        print("DIFFERS", line)
    print("the generators reproduce the fixtures" if not bad else f"{len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
