"""Summary of an A/B of two builds of the library on the headline step (RSN_LIBRARY, run as parent / this / this / parent per arm):
reads the bench.py result lines a job left under a directory and writes the per-arm comparison of profiles/normals_shape16.json
and profiles/backward_x9.json -- per figure the two runs of each build, their pair spreads, the fall and the fall over the sum of
the spreads -- and judges the criterion those records state.
  python tools/ab_library_report.py DIR --must-fall ms_per_step field_backward field_backward_input [--out FILE]
DIR holds <arm>_<k>_<parent|this>.json (k = run order 1..4), each with bench.py's JSON line last; <arm> names the bench command."""
import argparse
import glob
import json
import os
import re


def _line(path):
    with open(path) as fh:
        rows = [ln for ln in fh if ln.startswith("{")]
    return json.loads(rows[-1])


def _pair(parent, this):
    ps, ts = abs(parent[0] - parent[1]), abs(this[0] - this[1])
    fall = sum(parent) / 2 - sum(this) / 2
    return {"parent": [round(v, 4) for v in parent], "this": [round(v, 4) for v in this], "parent_spread_ms": round(ps, 4),
            "this_spread_ms": round(ts, 4), "fall_ms": round(fall, 4), "ratio_this_over_parent": round(sum(this) / sum(parent), 5),
            "fall_over_sum_of_spreads": round(fall / max(ps + ts, 1e-9), 1)}


def arm(dirname, name, must_fall):
    runs = {"parent": [], "this": []}
    for path in sorted(glob.glob(os.path.join(dirname, name + "_[0-9]_*.json"))):
        runs[re.search(r"_(parent|this)\.json$", path).group(1)].append(_line(path))
    assert len(runs["parent"]) == 2 and len(runs["this"]) == 2, (name, {k: len(v) for k, v in runs.items()})
    get = lambda f: _pair([f(j) for j in runs["parent"]], [f(j) for j in runs["this"]])  # noqa: E731
    ts = runs["parent"][0]["train_step"]
    out = {"order": "parent / this / this / parent", "ms_per_step": get(lambda j: j["ms_per_step"]),
           "launch_kinds_avg_launch_ms": {k: dict(launches_per_step=ts["launch_kinds"][k]["launches_per_step"],
                                                  **get(lambda j, k=k: j["train_step"]["launch_kinds"][k]["avg_launch_ms"]))
                                          for k in ts["launch_kinds"]},
           "kernels_ms_per_step": {k: get(lambda j, k=k: j["train_step"]["kernels"][k]["ms_per_step"]) for k in ts["kernels"]},
           "other_ms_per_step": get(lambda j: j["train_step"]["other_ms_per_step"])}
    figures = {"ms_per_step": out["ms_per_step"], "other_ms_per_step": out["other_ms_per_step"], **out["launch_kinds_avg_launch_ms"],
               **out["kernels_ms_per_step"]}
    out["slower_beyond_their_larger_pair_spread"] = {k: v["fall_ms"] for k, v in figures.items()
                                                     if -v["fall_ms"] > max(v["parent_spread_ms"], v["this_spread_ms"])}
    out["fell_by_more_than_the_sum_of_spreads"] = {k: figures[k]["fall_ms"] > figures[k]["parent_spread_ms"] + figures[k]["this_spread_ms"]
                                                   for k in must_fall}
    out["criterion_met"] = all(out["fell_by_more_than_the_sum_of_spreads"].values()) and not out["slower_beyond_their_larger_pair_spread"]
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--must-fall", nargs="+", default=["ms_per_step"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    names = sorted({re.match(r"(.+)_[0-9]_(parent|this)\.json$", os.path.basename(p)).group(1)
                    for p in glob.glob(os.path.join(a.dir, "*_[0-9]_*.json"))})
    rec = {n: arm(a.dir, n, a.must_fall) for n in names}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    for n in names:
        r = rec[n]
        print(n, "criterion met" if r["criterion_met"] else "criterion NOT met", "ms/step", r["ms_per_step"], "slower:", r["slower_beyond_their_larger_pair_spread"])
        for k in a.must_fall[1:]:
            print("  ", k, r["launch_kinds_avg_launch_ms"].get(k) or r["kernels_ms_per_step"].get(k))
