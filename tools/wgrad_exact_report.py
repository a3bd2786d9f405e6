"""Record how much of the entry-wise bound of tests/test_wgrad_exact_gpu.py (item 7) the weight-gradient kernels use on the device:
every random case is run once per flush, and per case the kernel's worst |err| / (2^-24 S) is written to profiles/wgrad_exact.json
beside the float32 restatement's worst ratio on the host and K = 4 x that, the bound's factor.  For the split-bf16 kernel the
segment lengths of the full-stage runs (item 2) are recorded with the wave slots' stage counts for this device's grid.  These are
measurements: they are recorded, and no bound is taken from them; no test reads the file.

    python tools/wgrad_exact_report.py [--out profiles/wgrad_exact.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from tests import test_wgrad_exact_gpu as T  # noqa: E402
from tests import wgrad_cases as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wgrad_exact.json"))
    args = ap.parse_args()
    pkg.load_library()
    dev = torch.device("cuda:0")
    rows, beyond = [], []
    for mode, n_out, k_in, ld_dy, ld_x in W.RANDOM_CASES:
        row = {"mode": mode, "n_out": n_out, "k_in": k_in, "ld_dy": ld_dy, "ld_x": ld_x}
        for flush in T.FLUSHES:
            ratio, K = T.random_ratio(dev, mode, n_out, k_in, ld_dy, ld_x, flush)
            row[flush] = round(ratio, 4)
            row["host_float32_restatement"], row["K"] = round(K / 4.0, 4), round(K, 4)
            if ratio > K:
                beyond.append(f"{mode} {n_out}x{k_in} {flush}")
        rows.append(row)
    stages = []
    for n_out, k_in in W.STAGE_SHAPES:
        nsub = W.nsub_of(n_out)
        lens, G = W.full_stage_lengths(lambda ls: T.launch_grid(dev, ls, n_out, k_in, n_out, k_in, "bf16x6"), nsub)
        hist, tails = T._histogram(lens, G, 16)
        stages.append({"n_out": n_out, "k_in": k_in, "segments": lens, "wave_slots": G, "tail_stages": tails,
                       "slot_segment_pairs_by_stage_count": {str(k): v for k, v in hist.items()}})
    res = {"device": torch.cuda.get_device_name(0), "points": sum(T.DT.LENS),
           "what": "worst |got - fp64| / (2^-24 S[n, k]), S = |dy|^T |x|, per random case of tests/test_wgrad_exact_gpu.py and flush; "
                   "host_float32_restatement: the same ratio of 16-point stage sums added in float32 on the host; K = 4 x that is the "
                   "test's bound.  Recorded, not used as bounds",
           "cases_beyond_K": beyond, "random_cases": rows, "full_stage_runs": stages}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
