"""Record how much of its derived bound rsn_ssim uses on the device: every case of tests/ssim_reference.py is run once, as
tests/test_ssim_gpu.py runs it, and per case the kernel's error against the float64 map, the float32 restatement's error, the bound
(4x that + 2^-24) and the ratio error / bound are written to profiles/ssim_edges.json.  These are measurements: they are recorded, and
no bound is taken from them.

    python tools/ssim_report.py [--out profiles/ssim_edges.json]"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from tests import ssim_reference as R  # noqa: E402
from tests import test_ssim_gpu as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "ssim_edges.json"))
    args = ap.parse_args()
    pkg.load_library()
    dev = torch.device("cuda:0")
    cases, worst, beyond = {}, {}, []
    for name in R.names():
        got, r = T.measure(dev, name)
        err = abs(got - r["ref"])
        ratio = err / r["bound"]
        cases[name] = {"height": R.CASES[name]["shape"][0] + R.HALO, "width": R.CASES[name]["shape"][1] + R.HALO,
                       "data_range": R.CASES[name]["data_range"], "float64": r["ref"], "kernel": got, "kernel_error": float(f"{err:.4g}"),
                       "float32_error": float(f"{r['f32_err']:.4g}"), "bound": float(f"{r['bound']:.4g}"), "ratio": round(ratio, 4)}
        cls = R.CASES[name]["class"]
        worst[cls] = max(worst.get(cls, 0.0), round(ratio, 4))
        if not err <= r["bound"]:
            beyond.append(name)
    res = {"device": torch.cuda.get_device_name(0), "cases": len(cases), "cases_beyond_their_bound": beyond,
           "what": "rsn_ssim against ssim_mean(float64) per case of tests/ssim_reference.py; bound = 4 x |ssim_mean(float32) - "
                   "ssim_mean(float64)| + 2^-24; ratio = kernel_error / bound; recorded, not used as bounds",
           "worst_ratio_per_class": worst, "per_case": cases}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: res[k] for k in ("device", "cases", "cases_beyond_their_bound", "worst_ratio_per_class")}, indent=1))


if __name__ == "__main__":
    main()
