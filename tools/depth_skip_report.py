"""Record how much of the derived bound of tests/layer_gemm_reference.py each GEMM of the training kernels uses on the nets of
tests/depth_skip_cases.py (trunk depths 1 .. 16, skip positions): every random-field case of tests/test_depth_skip_gpu.py
is run once, and per (family, net) the worst |err| / B of every record, the d_input and normals figures of
field_maths_reference.compare, the live share of each layer's units and the kernel family train_layout() reports are written to
profiles/depth_skip.json, with the cases judged by their integer case alone (test_depth_skip_gpu.INTEGER_ONLY).  These are
measurements: they are recorded, and no bound is taken from them.

    python tools/depth_skip_report.py [--out profiles/depth_skip.json] [--junit junit.xml]

--junit: the JUnit file of one `pytest tests -m gpu --junitxml=...` run; the time of the whole suite and the time of the tests this
file's subject added (tests/test_depth_skip_gpu.py and the depth / skip cases of test_gpu_parity's packing test) are recorded from it."""
import argparse
import json
import os
import re
import sys
import xml.etree.ElementTree as ET

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from tests import depth_skip_cases as D  # noqa: E402
from tests import test_depth_skip_gpu as T  # noqa: E402

ADDED = ("tests.test_depth_skip_gpu", "at_depth_and_skip_extremes")


def suite_times(path):
    """-> seconds of every test case of the JUnit file, and of the added ones among them"""
    total = added = 0.0
    n_total = n_added = 0
    for case in ET.parse(path).getroot().iter("testcase"):
        t = float(case.get("time", "0"))
        total, n_total = total + t, n_total + 1
        if case.get("classname", "").startswith(ADDED[0]) or ADDED[1] in case.get("name", ""):
            added, n_added = added + t, n_added + 1
    return {"gpu_tests": n_total, "gpu_tests_added": n_added, "seconds_after": round(total, 1), "seconds_before": round(total - added, 1),
            "seconds_added": round(added, 1), "what": "sum of the per-test times of one `pytest tests -m gpu` run; before = without the added tests"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_skip.json"))
    ap.add_argument("--junit", default=None)
    args = ap.parse_args()
    pkg.load_library()
    dev = torch.device("cuda:0")
    out, beyond = {}, []
    for family, fold, width, net, points in D.random_cases():
        r = T.random_case(dev, family, fold, width, net, points)
        fam = family + ("-fold" if fold else "")
        e = out.setdefault(f"{fam} w{width}", {}).setdefault(net, {"kernel": "ring" if r["ring"] else "per wave", "share_of_bound": {}})
        for k, v in r["shares"].items():
            k = re.sub(r"\[\d+\]", "", k)  # act[l], dy[l]: one entry, the worst layer
            e["share_of_bound"][k] = round(max(e["share_of_bound"].get(k, 0.0), v), 4)
        for name, verdict in (("d_input", r["d_input"]), ("normals", r["normals"])):
            if verdict is not None:
                row = verdict.rows[0]
                prev = e.get(name)
                if prev is None or row["got"] / max(row["bound"], 1e-300) > prev["kernel"] / max(prev["bound"], 1e-300):
                    e[name] = {"kernel": row["got"], "fp32_oracle": row["oracle"], "bound": row["bound"], "ok": row["ok"], "points": points}
                if not row["ok"]:
                    beyond.append({"case": r["label"], "quantity": name, "kernel": row["got"], "bound": row["bound"],
                                   "integer_only": (fam, net) in T.INTEGER_ONLY})
        e["live_share_per_layer"] = [round(s, 3) for s in r["live"]]
        if r["failures"] or r["bits"]:
            beyond.append({"case": r["label"], "records": r["failures"] + r["bits"]})
    res = {"device": torch.cuda.get_device_name(0), "cases": len(D.random_cases()),
           "what": "per (family, width) and net of tests/depth_skip_cases.py: worst |err| / B per record, d_input and normals under "
                   "field_maths_reference.compare, live share of units per layer; recorded, not used as bounds",
           "nets": {n: {"layers": l, "skip": D.skip_of(s)} for n, (l, s) in D.NETS.items()},
           "judged_by_the_integer_case_alone": [{"family": fa, "net": n, "quantity": q, "why": why} for (fa, n), (q, why) in T.INTEGER_ONLY.items()],
           "beyond_a_bound": beyond, "results": out}
    if args.junit:
        res["suite_time"] = suite_times(args.junit)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"beyond_a_bound": beyond, "suite_time": res.get("suite_time")}, indent=1))


if __name__ == "__main__":
    main()
