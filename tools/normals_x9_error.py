#!/usr/bin/env python3
"""Largest error of the analytic normals against the fp64 sweep on the 8 x 256 field (128 rays x 32 samples, the inputs of
tests/test_normals_x9_gpu.py::test_error_at_the_headline_width), with whatever library RSN_LIBRARY names -- run once per build
for the pair profiles/normals_x9.json records.
Usage: [RSN_LIBRARY=<librsn_hip.so>] python tools/normals_x9_error.py [out.json | -]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reflect_sampling_nerf_amd as pkg  # noqa: E402
from tests.test_normals_x9_gpu import worst_error  # noqa: E402

assert torch.cuda.is_available(), "needs an MI355X"
pkg.load_library()
res = {"library": os.environ.get("RSN_LIBRARY", "the tree's own"), "points": 4096}
for fold in (True, False):
    got, ref, ora = worst_error(torch.device("cuda:0"), fold)
    res["folded" if fold else "unfolded"] = {
        "worst_abs_error_vs_fp64": float((got.double() - ref).abs().max()),
        "mean_abs_error_vs_fp64": float((got.double() - ref).abs().mean()),
        "float32_restatement_worst_abs_error_vs_fp64": float((ora.double() - ref).abs().max()),
    }
out = sys.argv[1] if len(sys.argv) > 1 else "-"
text = json.dumps(res, indent=1)
if out == "-":
    print(text)
else:
    with open(out, "w") as fh:
        fh.write(text + "\n")
