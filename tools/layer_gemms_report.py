"""Record how much of the derived bound of tests/layer_gemm_reference.py each GEMM of the training kernels uses on the device: every
case of tests/test_layer_gemms_gpu.py is run once, and per family and record the worst |err| / B over all cases is written to
profiles/layer_gemms.json (d_input: the kernel's worst error over the bound of field_maths_reference.compare).  These are
measurements: they are recorded, and no bound is taken from them.

    python tools/layer_gemms_report.py [--out profiles/layer_gemms.json]"""
import argparse
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from tests import test_layer_gemms_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "layer_gemms.json"))
    args = ap.parse_args()
    pkg.load_library()
    dev = torch.device("cuda:0")
    out, n_cases, failed = {}, 0, []

    def book(family, fold, r):
        fam = out.setdefault(family + ("_folded" if fold else ""), {})
        for k, v in r["shares"].items():
            k = re.sub(r"\[\d+\]", "", k)  # act[l], dy[l]: one entry, the worst layer
            fam[k] = max(fam.get(k, 0.0), v)
        d = r["d_input"].rows[0]
        fam["d_input"] = max(fam.get("d_input", 0.0), d["got"] / d["bound"] if d["bound"] > 0 else float(d["got"] > 0))
        if r["failures"] or not r["d_input"].ok:
            failed.append(r["label"])

    for family, fold, width, net, points in T.CASES:
        book(family, fold, T.run_case(dev, family, fold, width, net, T.POINTS[points]))
        n_cases += 1
    for family, fold, width in T.COUNT_CASES:
        book(family, fold, T.run_case(dev, family, fold, width, "L8", (60, 3), n_live_rays=47))
        n_cases += 1
    for family, fold, width in T.INF_CASES:
        for r in T.run_inf_case(dev, family, fold, width):
            book(family, fold, r)
        n_cases += 1
    res = {"device": torch.cuda.get_device_name(0), "cases": n_cases, "cases_beyond_a_bound": failed,
           "what": "worst |err| / B per family and record over every case of tests/test_layer_gemms_gpu.py; recorded, not used as bounds",
           "share_of_bound": {f: {k: round(v, 4) for k, v in sorted(r.items())} for f, r in out.items()}}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res["share_of_bound"], indent=1))


if __name__ == "__main__":
    main()
