#!/usr/bin/env python3
"""Compares two `bench.py --dump-outputs DIR` directories array for array, BIT for bit (the bytes of each .npy payload).
Two runs of one build with RSN_DETERMINISTIC=1 must come out identical in every array; without it the parameter gradients
differ in their last bits (the weight-gradient atomics).  Exit status 1 if any array differs or is missing on one side.
    python tools/dump_bitcmp.py DIR_A DIR_B"""
import os
import sys

import numpy as np


def main(a, b):
    names_a = {f for f in os.listdir(a) if f.endswith(".npy")}
    names_b = {f for f in os.listdir(b) if f.endswith(".npy")}
    differ, worst = [], 0.0
    for f in sorted(names_a & names_b):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            rel = float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max() / max(np.abs(x).max(), 1e-30)) if x.shape == y.shape else float("inf")
            worst = max(worst, rel)
            differ.append((f, rel))
    for f, rel in differ:
        print(f"DIFFERS {f}: max |a - b| / max |a| = {rel:.3e}")
    only = sorted(names_a ^ names_b)
    for f in only:
        print(f"ONLY ON ONE SIDE {f}")
    n = len(names_a & names_b)
    print(f"{n - len(differ)} of {n} arrays bit-identical" + (f", worst relative difference {worst:.3e}" if differ else ""))
    return 1 if differ or only or n == 0 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
