#!/usr/bin/env python3
"""Records tests/golden/ppo_update_bits.npz: the state PPONet.ppo_update leaves behind, bit for bit, for the sequences of
tests/ppo_update_bits_cases.py (needs an MI355X and a built library).

Run it at the commit whose arithmetic is to be pinned -- BEFORE a change that claims to keep every bit -- and commit the file with that change;
tests/test_ppo_update_bits_gpu.py replays the same calls against it.  --check records again and compares with the file instead of writing it
(two recordings of one commit must be identical, else the update is not deterministic and the fixture proves nothing).

Usage:  python tools/gen_ppo_update_bits.py [--out tests/golden/ppo_update_bits.npz] [--check]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ppo_update_bits_cases as BC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ppo_update_bits.npz"))
    ap.add_argument("--check", action="store_true", help="record again and compare with --out instead of writing it")
    a = ap.parse_args()
    rec = BC.run_all()
    if a.check:
        old = np.load(a.out)
        bad = [k for k in rec if k not in old.files or not np.array_equal(old[k].view(np.uint8), rec[k].view(np.uint8))]
        bad += [k for k in old.files if k not in rec]
        print(f"{a.out}: {len(rec)} arrays recorded again, {len(bad)} differ" + (": " + ", ".join(bad[:8]) if bad else " -- identical"))
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **rec)
    print(f"{a.out}: {len(rec)} arrays, {os.path.getsize(a.out)} bytes")
    for c in BC.CASES:
        print(f"  {c.name}: loss after each call {rec[c.name + '/stats'][:, 0]}, step {rec[c.name + '/hyper'][:, 4]}")


if __name__ == "__main__":
    main()
