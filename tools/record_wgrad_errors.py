#!/usr/bin/env python
"""Records tests/golden/wgrad_errors.json: what the weight-gradient entry points of include/rsn.h answer to invalid arguments --
(return code, rsn_last_error()) -- to the calls that return RSN_OK without work (no segments, or every segment empty) and to the
launches they refuse before launching (bf16 operand rows in a mode or a layout that no kernel reads, an ordered call without its
workspace).  No case reaches a launch, so no GPU is needed; the process hides the GPUs from itself so that a library that lets one
through fails with RSN_ERR_HIP (which the matrix refuses) and cannot launch a kernel on the made-up pointers used here.

Per entry point: a valid argument set, each single edit of it and every PAIR of edits (a pair shows which of two checks comes first).
  * The atomic entry points are never called with an argument set they would launch: where no edit of a case is an error by itself,
    every segment is emptied as well and the call returns RSN_OK without work.
  * The ordered entry points always get workspace_bytes = 0: a call that passes every other check stops at the size check, whose
    message ("needs N bytes") pins the grid of the launch.  (One case has a workspace that is large enough, and is refused behind it.)
  * rsn_weight_grad_workspace_bytes: (0, message) on failure, (bytes, "") otherwise -- with the GPUs hidden, for 256 CUs.
The *_jobs entry points take the row edits in job 0 and in job 1 of a two-job launch.

Usage: RSN_LIBRARY=<librsn_hip.so of the commit to pin> python tools/record_wgrad_errors.py [out.json | -] [--bound '<shapes>']
--bound '[[n_out, k_in, ld_dy, ld_x], ...]' adds "workspace_bound": per shape, mode 0..3, list of segment lengths and X alignment,
[case, bytes the ordered launch asks for, rsn_weight_grad_workspace_bytes of the same arguments] (see workspace_bound).
tests/test_abi_cpu.py::test_weight_grad_argument_errors_are_pinned replays the matrix on the tree's own build."""
import ctypes as C
import hashlib
import itertools
import json
import os
import re
import sys

for _v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):  # before the HIP runtime loads
    os.environ[_v] = "-1" if _v != "ROCR_VISIBLE_DEVICES" else ""

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflect_sampling_nerf_amd import _abi  # noqa: E402

RSN_ERR_HIP = -3
WG_MAX_SEG, WG_MAX_JOBS = 8, 8
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "wgrad_errors.json")
_next = itertools.count(1)


def fake():
    """A distinct non-NULL address, 4 KiB aligned: checked against NULL and for alignment on the host, never dereferenced there."""
    return 0x100000 + 0x1000 * next(_next)


def valid(n_jobs):
    """The logical arguments of a valid call: three segments, the middle one empty, the first two with a device-side count."""
    job = lambda: {"dy": [fake(), fake(), fake()], "x": [fake(), fake(), fake()], "dw": fake(), "ld_dw": 72, "db": fake()}  # noqa: E731
    return {"_ns": 3, "n_segments": 3, "n_points": [40, 0, 24], "n_dev": [fake(), fake(), None], "per_count": [4, 4, 4], "ld_dy": 64, "n_out": 64,
            "ld_x": 64, "k_in": 64, "mma_mode": 0, "operand_bf16": 0, "workspace": fake(), "workspace_bytes": 0, "n_jobs": n_jobs,
            "jobs": [job() for _ in range(n_jobs)]}


def call(lib, fn, p):
    """Calls entry point `fn` with the logical arguments p; a member that is None goes as NULL."""
    ns = p["_ns"]  # the length of the arrays, whatever n_segments says
    arr = lambda t, v: None if v is None else (t * ns)(*v)  # noqa: E731
    npts, ndev, per = arr(C.c_int64, p["n_points"]), arr(C.c_void_p, p["n_dev"]), arr(C.c_int32, p["per_count"])
    rows = [(arr(C.c_void_p, q["dy"]), arr(C.c_void_p, q["x"])) for q in p["jobs"] or []]
    shape = (p["ld_dy"], p["n_out"], p["ld_x"], p["k_in"])
    how = (p["mma_mode"], p["operand_bf16"])
    ws = (p["workspace"], p["workspace_bytes"])
    f = getattr(lib, fn)
    if fn == "rsn_weight_grad_workspace_bytes":
        return f(p["n_segments"], npts, p["n_jobs"], p["n_out"], p["k_in"], *how)
    if "jobs" in fn:
        jobs = None
        if p["jobs"] is not None:
            jobs = (_abi.WGradJob * len(p["jobs"]))()
            for q, src, (dys, xs) in zip(jobs, p["jobs"], rows):
                q.dy, q.x, q.col_map, q.dw, q.ld_dw, q.db = dys, xs, None, src["dw"], src["ld_dw"], src["db"]
        return f(p["n_segments"], npts, ndev, per, p["n_jobs"], jobs, *shape, *how, *(ws if "ordered" in fn else ()), None)
    q, (dys, xs) = p["jobs"][0], rows[0]  # the flat entry points: job 0 is the call's rows and outputs
    if fn == "rsn_weight_grad":
        return f(p["n_points"][0], dys and dys[0], shape[0], shape[1], xs and xs[0], shape[2], shape[3], None, q["dw"], q["ld_dw"], q["db"],
                 None)
    flat = (dys, shape[0], shape[1], xs, shape[2], shape[3], None, q["dw"], q["ld_dw"], q["db"])
    if fn == "rsn_weight_grad_multi":
        return f(p["n_segments"], npts, *flat, None)
    if fn == "rsn_weight_grad_multi_mode":
        return f(p["n_segments"], npts, *flat, p["mma_mode"], None)
    return f(p["n_segments"], npts, ndev, per, *flat, *how, *(ws if "ordered" in fn else ()), None)


def edit(label, kind="hard", **members):
    """An edit: members of the logical arguments to set ("jobs.K.name" / "name.I" reach into job K / element I).  kind "hard": an
    error whatever else the call says; "soft": no error by itself; "refused": a launch-time refusal, complete in itself."""
    return (label, kind, members)


def apply(p, members):
    for path, value in members.items():
        at, keys = p, [int(k) if k.isdigit() else k for k in path.replace("__", ".").split(".")]
        for k in keys[:-1]:
            at = at[k]
        at[keys[-1]] = value


ENTRY_POINTS = ("rsn_weight_grad", "rsn_weight_grad_multi", "rsn_weight_grad_multi_mode", "rsn_weight_grad_multi_dev",
                "rsn_weight_grad_multi_dev_ordered", "rsn_weight_grad_jobs", "rsn_weight_grad_jobs_ordered",
                "rsn_weight_grad_workspace_bytes")


def edits_of(fn):
    single, size = fn == "rsn_weight_grad", fn == "rsn_weight_grad_workspace_bytes"
    jobs, dev, ordered = "jobs" in fn, "dev" in fn or "jobs" in fn, "ordered" in fn
    e = [edit("n_out=0", n_out=0), edit("n_out=257", n_out=257), edit("k_in=0", k_in=0), edit("k_in=257", k_in=257)]
    if single:
        e += [edit("n_points=-1", n_points__0=-1), edit("n_points=0", "soft", n_points__0=0)]
    else:
        e += [edit("n_segments=-1", n_segments=-1), edit("n_segments=9", n_segments=WG_MAX_SEG + 1),
              edit("n_segments=0", "soft", n_segments=0), edit("n_points=NULL", n_points=None), edit("n_points[2]=-1", n_points__2=-1),
              edit("every segment empty", "soft", n_points=[0, 0, 0])]
    if size:
        e += [edit("n_jobs=0", n_jobs=0), edit("n_jobs=9", n_jobs=WG_MAX_JOBS + 1)]
    else:
        e += [edit("ld_dy=n_out-1", ld_dy=63), edit("ld_x=k_in-1", ld_x=63)]
    if dev or size or fn == "rsn_weight_grad_multi_mode":
        e += [edit("mma_mode=-1", mma_mode=-1), edit("mma_mode=4", mma_mode=4)]
        e += [edit("mma_mode=%d" % m, "soft", mma_mode=m) for m in (1, 2, 3)]
    if dev or size:
        e += [edit("operand_bf16=-1", operand_bf16=-1), edit("operand_bf16=4", operand_bf16=4)]
    if dev:
        counts = "soft" if jobs else "hard"  # the flat entry points require both arrays, the jobs ones take "no counts"
        e += [edit("n_dev=NULL", counts, n_dev=None), edit("per_count=NULL", counts, per_count=None), edit("per_count[0]=0", per_count__0=0),
              edit("per_count[2]=0 (no count)", "soft", per_count__2=0)]
        # the refusals of a launch whose arguments are in range: bf16 rows outside RSN_MMA_BF16 ...
        e += [edit("bf16 rows %d, mma_mode %d" % (o, m), "refused", operand_bf16=o, mma_mode=m) for o in (1, 2, 3) for m in (0, 1)]
        # ... or off the vector-load layout (X: k_in % NKB, ld_x % NKB, 2 NKB-byte rows; dY: n_out > 32, even ld_dy, 4-byte rows) ...
        bf = {"mma_mode": 3}
        for k in ([0, 1] if jobs else [0]):
            at = "jobs.%d." % k
            tag = "job %d: " % k if jobs else ""
            e += [edit(tag + "bf16 X rows, x[2] + 2 bytes", "refused", operand_bf16=1, n_out=32, ld_dy=32, **bf, **{at + "x.2": fake() + 2}),
                  edit(tag + "bf16 dY rows, dy[0] + 2 bytes", "refused", operand_bf16=2, **bf, **{at + "dy.0": fake() + 2})]
        e += [edit("bf16 X rows, k_in=63", "refused", operand_bf16=1, n_out=32, ld_dy=32, k_in=63, **bf),
              edit("bf16 X rows, ld_x=65", "refused", operand_bf16=1, n_out=32, ld_dy=32, ld_x=65, **bf),
              edit("bf16 dY rows, n_out=32", "refused", operand_bf16=2, n_out=32, **bf),
              edit("bf16 dY rows, ld_dy=65", "refused", operand_bf16=3, ld_dy=65, **bf)]
        # ... or bf16 X beside fp32 dY of more than 32 outputs, which no kernel reads (behind the workspace checks)
        e += [edit("bf16 X rows, fp32 dY rows, n_out=64", "refused", operand_bf16=1, workspace_bytes=1 << 40, **bf)]
    if ordered:
        e += [edit("workspace=NULL", workspace=None), edit("workspace + 8 bytes", workspace=fake() + 8)]
    if jobs:
        e += [edit("n_jobs=0", n_jobs=0), edit("n_jobs=9", n_jobs=WG_MAX_JOBS + 1), edit("jobs=NULL", jobs=None)]
    for k in ([0, 1] if jobs else [] if size else [0]):
        at, tag = "jobs.%d." % k, "job %d: " % k if jobs else ""
        e += [edit(tag + m + "=NULL", **{at + m: None}) for m in ("dy", "x", "dw")] + [edit(tag + "ld_dw=0", **{at + "ld_dw": 0})]
        if not single:
            e += [edit(tag + "dy[0]=NULL", **{at + "dy.0": None}), edit(tag + "x[2]=NULL", **{at + "x.2": None}),
                  edit(tag + "dy[1]=NULL (empty segment)", "soft", **{at + "dy.1": None})]
    return e


def roots(members):
    """What two edits must not both touch: the argument, or the member of the job (n_dev and per_count count as one: a count that is
    not there makes its per_count moot)."""
    return {".".join(path.replace("__", ".").split(".")[:3 if path.startswith("jobs.") else 1]).replace("per_count", "n_dev")
            for path in members}


def record(lib, results, name, fn, p):
    rc = call(lib, fn, p)
    failed = rc == 0 if fn == "rsn_weight_grad_workspace_bytes" else rc != 0
    msg = lib.rsn_last_error().decode() if failed else ""  # not cleared on success
    assert rc != RSN_ERR_HIP, "%s reached the device: %s" % (name, msg)
    assert name not in results, name
    results[name] = [rc, msg]


def wgrad_error_matrix(lib):
    results = {}
    for fn in ENTRY_POINTS:
        edits = edits_of(fn)
        stops = "ordered" in fn or fn == "rsn_weight_grad_workspace_bytes"  # a call in range does not launch
        if stops:
            record(lib, results, fn + " | in range", fn, valid(2 if "jobs" in fn else 1))
        for combo in [(e,) for e in edits] + list(itertools.combinations(edits, 2)):
            touched = [r for e in combo for r in roots(e[2])]
            if len(set(touched)) < len(touched) or ("jobs" in touched and any(t.startswith("jobs.") for t in touched)):
                continue  # two values of one argument
            p = valid(2 if "jobs" in fn else 1)
            label = " & ".join(e[0] for e in combo)
            for e in combo:
                apply(p, e[2])
            if not stops and all(e[1] == "soft" for e in combo) and p["n_segments"] != 0 and any(p["n_points"]):
                # nothing here is an error by itself: the call gets no points
                p["n_points"], label = [0] * len(p["n_points"]), label + " (no points)"
            record(lib, results, fn + " | " + label, fn, p)
    return results


def workspace_bound(lib, shapes):
    """[case, N, bound]: N from "needs N bytes" of rsn_weight_grad_multi_dev_ordered with workspace_bytes = 0, bound =
    rsn_weight_grad_workspace_bytes of the same segments, shape and mode; X rows aligned, and 4 bytes off (the scalar-load grid)."""
    out = []
    for (n_out, k_in, ld_dy, ld_x), mode, lens, off in itertools.product(
            shapes, range(4), ([8], [1000, 0, 37, 5003, 3], [10 ** 6], [300000, 300000, 524288]), (0, 4)):
        p = valid(1)
        n = len(lens)
        q = {"dy": [fake() for _ in lens], "x": [fake() + off for _ in lens], "dw": fake(), "ld_dw": k_in, "db": fake()}
        p.update(_ns=n, n_segments=n, n_points=lens, n_dev=[None] * n, per_count=[1] * n, ld_dy=ld_dy, n_out=n_out, ld_x=ld_x, k_in=k_in,
                 mma_mode=mode, jobs=[q])
        name = "%dx%d ld %d/%d mode %d lens %s x+%d" % (n_out, k_in, ld_dy, ld_x, mode, lens, off)
        rc = call(lib, "rsn_weight_grad_multi_dev_ordered", p)
        msg = lib.rsn_last_error().decode()
        m = re.search(r"needs (\d+) bytes", msg)
        assert rc == -1 and m, "%s: %d %s" % (name, rc, msg)
        out.append([name, int(m.group(1)), int(call(lib, "rsn_weight_grad_workspace_bytes", p))])
    return out


def cases_digest(names):
    return hashlib.sha256("\n".join(sorted(names)).encode()).hexdigest()


def write_golden(path, doc):
    """The compact record: the distinct answers, the digest of the sorted case names (`python tools/record_wgrad_errors.py -` lists
    them) and, in that order, each case's index into the answers."""
    idx = [doc["cases"][k] for k in sorted(doc["cases"])]
    rows = [", ".join(map(str, idx[i:i + 50])) for i in range(0, len(idx), 50)]
    with open(path, "w") as fh:
        fh.write('{"answers": [\n' + ",\n".join(json.dumps(a) for a in doc["answers"]) + '],\n"n_cases": %d,\n"cases_sha256": "%s",\n'
                 % (len(idx), cases_digest(doc["cases"])) + '"answer_of_case": [\n' + ",\n".join(rows) + "]}\n")


if __name__ == "__main__":
    argv = sys.argv[1:]
    shapes = json.loads(argv.pop(argv.index("--bound") + 1)) if "--bound" in argv else None
    argv = [a for a in argv if a != "--bound"]
    out = argv[0] if argv else GOLDEN
    library = _abi.load_library()
    res = wgrad_error_matrix(library)
    # the few dozen distinct (return code, message) pairs are stored once; stdout gets {case: index into "answers"}, the golden file
    # the indices alone, in the order of the sorted case names, with the names' digest (write_golden)
    answers = sorted(set(map(tuple, res.values())), key=lambda a: (-a[0], a[1]))
    doc = {"answers": answers, "cases": {k: answers.index(tuple(v)) for k, v in sorted(res.items())}}
    if shapes is not None:
        doc["workspace_bound"] = workspace_bound(library, shapes)
    if out == "-":
        sys.stdout.write(json.dumps(doc, indent=0) + "\n")
    else:
        write_golden(out, doc)
        print("%d cases -> %s (library: %s)" % (len(res), out, os.environ.get("RSN_LIBRARY", "the tree's own")), file=sys.stderr)
