"""Record how much of their bounds the samplers, the standalone encoders and the RAdam step use on the device.  The tests print one line
per check, quantity and class -- "[case] quantity class: kernel E (...), fp32 oracle E, bound E" (field_maths_reference.compare's verdict) --
and "RATIO name value [case] (bound B, ...)" for the sums of tests/test_render_ops_gpu.py; this tool parses those lines out of a pytest log
and writes, per quantity and class, the worst kernel error, the float32 oracle's, the bound and the kernel's share of the bound to
profiles/step_edges.json, with the share of samples each PDF case left out.  These are measurements: no bound is taken from them.

    python -m pytest -s -q tests/test_samplers_gpu.py tests/test_radam_gpu.py tests/test_encoders_gpu.py \\
        "tests/test_render_ops_gpu.py::test_loss_scale_grads_on_fused_loss_buffers" > step_edges.log
    python tools/step_edges_report.py step_edges.log [--out profiles/step_edges.json] [--device NAME]"""
import argparse
import json
import os
import re

QUANTITIES = ("spaced spacing bins", "spaced euclidean bins", "pdf spacing bins", "pdf euclidean bins", "pdf euclidean map", "radam p", "radam m",
              "radam v", "ipe_encode", "sh34_encode")
LINE = re.compile(r"^\.*\[(?P<case>[^\]]*)\] (?P<q>" + "|".join(QUANTITIES) + r") (?P<cls>\S+): kernel (?P<got>\S+) \((?P<where>[^)]*)\), "
                  r"fp32 oracle (?P<oracle>\S+), bound (?P<bound>\S+?)(?P<fail>\s+<-- FAIL)?$")
RATIO = re.compile(r"^\.*RATIO (?P<name>\S+) (?P<ratio>\S+) \[(?P<case>[^\]]*)\] \(bound (?P<bound>[0-9.]+),")
EXCLUDED = re.compile(r"^\.*EXCLUDED (?P<case>\S+): (?P<share>[0-9.]+)% \(cap")
RADAM_CLASS = re.compile(r"^g_(1e-?\d+|zero)$")


def parse(lines):
    checks, ratios, excluded, beyond = {}, {}, {}, set()
    for line in lines:
        line = line.rstrip("\n")
        m = LINE.match(line)
        if m:
            q, cls = m["q"], m["cls"]
            if q.startswith("radam") and RADAM_CLASS.match(cls):
                cls = "all gradient decades"  # 16 classes per quantity: the worst one is recorded
            if q in ("ipe_encode", "sh34_encode"):
                cls = "all input classes"
            got, oracle, bound = float(m["got"]), float(m["oracle"]), float(m["bound"])
            share = got / bound if bound > 0 else float(got > 0)
            e = checks.setdefault(q, {}).setdefault(cls, {"share_of_bound": -1.0, "lines": 0})
            e["lines"] += 1
            if share > e["share_of_bound"]:
                e.update({"share_of_bound": share, "kernel": got, "fp32_oracle": oracle, "bound": bound, "case": m["case"], "where": m["where"]})
            if m["fail"]:
                beyond.add(f"{m['case']}: {q} {m['cls']}")
            continue
        m = RATIO.match(line)
        if m:
            r = ratios.setdefault(m["name"], {"worst_ratio_x_2^-24": 0.0, "bound_x_2^-24": float(m["bound"])})
            if float(m["ratio"]) > r["worst_ratio_x_2^-24"]:
                r.update({"worst_ratio_x_2^-24": float(m["ratio"]), "case": m["case"]})
            if float(m["ratio"]) > float(m["bound"]):
                beyond.add(f"{m['case']}: {m['name']} {m['ratio']} x 2^-24 of the scale, bound {m['bound']}")
            continue
        m = EXCLUDED.match(line)
        if m:
            excluded[m["case"]] = round(float(m["share"]) / 100.0, 8)
    return checks, ratios, excluded, sorted(beyond)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("log", help="output of pytest -s on the four test files")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "step_edges.json"))
    ap.add_argument("--device", default="AMD Instinct MI355X")
    args = ap.parse_args()
    with open(args.log) as fh:
        checks, ratios, excluded, beyond = parse(fh)
    for q in checks.values():
        for e in q.values():
            for k in ("share_of_bound", "kernel", "fp32_oracle", "bound"):
                e[k] = float(f"{e[k]:.4g}")
    res = {"device": args.device,
           "what": "worst share of its bound per quantity and class over every printed check of tests/test_samplers_gpu.py, test_radam_gpu.py, "
                   "test_encoders_gpu.py and the fused-loss cases of test_render_ops_gpu.py; recorded, not used as bounds",
           "checks_beyond_a_bound": beyond, "checks": {q: dict(sorted(c.items())) for q, c in sorted(checks.items())},
           "sums": ratios, "pdf_samples_left_out": {"cap": 0.005, "worst": max(excluded.values(), default=0.0),
                                                    "cases_with_any": {k: v for k, v in sorted(excluded.items()) if v > 0}}}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({q: {c: e["share_of_bound"] for c, e in cs.items()} for q, cs in res["checks"].items()}, indent=1))
    print(json.dumps(res["sums"], indent=1))


if __name__ == "__main__":
    main()
