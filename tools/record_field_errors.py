#!/usr/bin/env python
"""Records tests/golden/field_errors.json: what every field entry point of include/rsn.h (eight forward, three backward) answers to
invalid arguments -- (return code, rsn_last_error()) -- and to the calls that return RSN_OK without work (no rays).  Every case returns
before the first HIP call, so no GPU is needed; the process hides the GPUs from itself so that a library that lets one through fails
with RSN_ERR_HIP (which the matrix refuses) and cannot launch a kernel on the made-up pointers used here.

Per entry point: a valid argument set (never called as it is), each single edit of it -- every required pointer NULL, every required
member of the structs NULL, the counts out of range -- and every PAIR of edits: a pair shows which of two checks comes first.  The
*_jobs entry points take the edits in job 0 and in job 1 of a two-job launch, and n_jobs out of range.

Usage: RSN_LIBRARY=<librsn_hip.so of the commit to pin> python tools/record_field_errors.py [out.json | -]
tests/test_abi_cpu.py::test_field_argument_errors_are_pinned replays the matrix on the tree's own build."""
import ctypes as C
import itertools
import json
import os
import sys

for _v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):  # before the HIP runtime loads
    os.environ[_v] = "-1" if _v != "ROCR_VISIBLE_DEVICES" else ""

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reflect_sampling_nerf_amd import _abi  # noqa: E402

RSN_MAX_JOBS = 3
RSN_ERR_HIP = -3
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "field_errors.json")
_next = itertools.count(1)


def fake():
    """A distinct non-NULL address: checked against NULL on the host, never dereferenced there."""
    return 0x100000 + 0x1000 * next(_next)


def filled(cls, names=None):
    st = cls()
    for name, _ in cls._fields_:
        if names is None or name in names:
            setattr(st, name, fake())
    return st


def make_desc(width=256, mode=_abi.RSN_MMA_F32):
    d = _abi.FieldDesc()
    d.num_layers, d.width, d.skip_layer, d.mid_width, d.density_bias, d.mma_mode = 8, width, 4, 128, 0.5, mode
    for i in range(16):
        d.freqs[i] = 2.0 ** (16.0 * i / 15.0)
    return d


SAVED_REQUIRED = ("enc", "act", "bott", "sh", "hid", "heads", "relu_bits")


class Case:
    """One call: plain arguments by name plus the structs they point to; `edit(path, value)` changes one of them."""

    def __init__(self, fn, order, args, structs):
        self.fn, self.order, self.args, self.structs = fn, order, dict(args), structs

    def edit(self, path, value):
        if "." in path:
            st, member = path.split(".")
            setattr(self.structs[st], member, value)
        else:
            self.args[path] = value

    def call(self, lib):
        argv = []
        for name in self.order:
            v = self.args[name]
            argv.append(C.byref(self.structs[name]) if v == "struct" else v)
        return getattr(lib, self.fn)(*argv)


def frustum_args(n_rays=5):
    return {"n_rays": n_rays, "n_dev": None, "n_samples": 7, "origins": fake(), "directions": fake(), "pixel_area": fake(),
            "euclid_bins": fake()}


def single_cases():
    """name -> (factory of a fresh valid Case, [edits: (label, path, value) + ("soft",) if the edit alone leaves the call valid])."""
    null = lambda *names: [(n + "=NULL", n, None) for n in names]  # noqa: E731
    saved = [("saved." + m + "=NULL", "saved." + m, None) for m in SAVED_REQUIRED]
    frustum_edits = null("origins", "directions", "pixel_area", "euclid_bins") + [
        ("n_samples=0", "n_samples", 0), ("n_rays=-1", "n_rays", -1), ("n_rays=0", "n_rays", 0, "soft")]
    inf_edits = [("n_rays=-1", "n_rays", -1), ("n_rays=0", "n_rays", 0, "soft")]
    common = null("desc", "packed") + [("desc.width=100", "desc.width", 100)]
    out = {}

    def add(fn, order, args, structs, edits):
        def factory():
            a = {k: (v() if callable(v) else v) for k, v in args.items()}
            s = {k: v() for k, v in structs.items()}
            return Case(fn, order, {**a, **{k: "struct" for k in s}, "packed": fake(), "stream": None}, s)
        out[fn] = (factory, common + edits)

    S = {"desc": make_desc, "out": lambda: filled(_abi.FieldOutputs), "saved": lambda: filled(_abi.FieldSaved)}
    fr = {k: (fake if k in ("origins", "directions", "pixel_area", "euclid_bins") else v) for k, v in frustum_args().items()}
    add("rsn_field_forward_frustum", ["desc", "packed", *fr, "out", "stream"], fr, {k: S[k] for k in ("desc", "out")},
        frustum_edits + null("out"))
    add("rsn_field_forward_frustum_train", ["desc", "packed", *fr, "out", "saved", "stream"], fr, S,
        frustum_edits + null("out", "saved") + saved)
    inf = {"n_rays": 5, "n_dev": None, "directions": fake, "sqradius": fake, "out_rgb": fake}
    add("rsn_field_forward_inf", ["desc", "packed", *inf, "stream"], inf, {"desc": make_desc},
        inf_edits + null("directions", "sqradius", "out_rgb"))
    add("rsn_field_forward_inf_train", ["desc", "packed", *inf, "saved", "stream"], inf, {k: S[k] for k in ("desc", "saved")},
        inf_edits + null("directions", "sqradius", "out_rgb", "saved") + saved)
    pts = [("n_points=-1", "n_points", -1), ("n_points=0", "n_points", 0, "soft")]
    gs = {"n_points": 5, "means": fake, "cov_diag": fake, "view_dirs": fake}
    add("rsn_field_forward_gaussians", ["desc", "packed", *gs, "out", "embedding", "stream"], {**gs, "embedding": None},
        {k: S[k] for k in ("desc", "out")}, pts + null("means", "out"))
    add("rsn_field_forward_gaussians_train", ["desc", "packed", *gs, "out", "embedding", "saved", "stream"],
        {**gs, "embedding": None}, S, pts + null("means", "out", "saved") + saved + [("desc.mma_mode=bf16", "desc.mma_mode", 3)])
    em = {"n_points": 5, "embedding": fake, "view_dirs": fake, "roughness": None}
    add("rsn_field_forward_embedding", ["desc", "packed", *em, "out", "stream"], em, {k: S[k] for k in ("desc", "out")},
        pts + null("embedding", "out"))
    B = {**S, "fwd": S["out"], "gin": lambda: filled(_abi.FieldGradsIn, ("sigma", "color", "weights")),
         "gout": lambda: filled(_abi.FieldGradsOut)}
    # what the sweeps require of the blocks is checked for every job, with or without rays: the edits that are legal alone ("soft")
    # are recorded on a call without rays, which an accepted argument set ends with RSN_OK and no work
    bwd_members = [(p + "=NULL", p, None) for p in ("saved.relu_bits", "saved.heads", "gout.dy")]
    bwd_members += [(p + "=NULL", p, None, "soft") for p in ("saved.enc", "gout.d_input")]
    bwd_members += [("need_input_grad=0", "need_input_grad", 0, "soft")]
    fused = [("gin.ray_pn_loss", "gin.ray_pn_loss", 0xABC000, "soft"), ("gin.ray_ori_loss", "gin.ray_ori_loss", 0xABD000, "soft")]
    fused += [(p + "=NULL", p, None, "soft") for p in ("gin.weights", "saved.normals", "fwd.pred_normals", "fwd.n_dot_d")]
    fwd_vals = [(p + "=NULL", p, None) for p in ("fwd.raw_density", "fwd.diff", "fwd.tint")]
    add("rsn_field_backward_frustum", ["desc", "packed", *fr, "fwd", "saved", "gin", "gout", "need_input_grad", "stream"],
        {**fr, "need_input_grad": 1}, {k: B[k] for k in ("desc", "fwd", "saved", "gin", "gout")},
        frustum_edits + null("fwd", "saved", "gin", "gout") + bwd_members + fwd_vals + fused)
    bi = {"n_rays": 5, "n_dev": None, "directions": fake, "sqradius": fake}
    add("rsn_field_backward_inf", ["desc", "packed", *bi, "saved", "g_rgb", "gout", "need_input_grad", "stream"],
        {**bi, "g_rgb": fake, "need_input_grad": 1}, {k: B[k] for k in ("desc", "saved", "gout")},
        inf_edits + null("directions", "sqradius", "g_rgb", "saved", "gout") + bwd_members)
    return out


def run_singles(lib, results):
    for fn, (factory, edits) in single_cases().items():
        combos = [(e,) for e in edits] + list(itertools.combinations(edits, 2))
        for combo in combos:
            paths = [e[1] for e in combo]
            if len(set(paths)) < len(paths):
                continue  # two values of one argument
            case = factory()
            label = " & ".join(e[0] for e in combo)
            if all(len(e) > 3 for e in combo):  # nothing here is an error by itself: the call gets no rays
                rays = "n_rays" if "n_rays" in case.args else "n_points"
                if rays not in paths:
                    combo, label = combo + ((None, rays, 0),), label + " (no rays)"
            # a member of a struct whose pointer is also NULL cannot be edited apart; the pointer edit goes last
            for _, path, value, *_ in sorted(combo, key=lambda e: "." not in e[1]):
                if "." in path and path.split(".")[0] not in case.structs:
                    break
                if value is None and "." not in path and case.args.get(path) == "struct":
                    case.args[path] = None
                else:
                    case.edit(path, value)
            else:
                record(lib, results, fn + " | " + label, case.call)


def record(lib, results, name, call):
    rc = call(lib)
    msg = lib.rsn_last_error().decode() if rc != 0 else ""
    assert rc != RSN_ERR_HIP, "%s reached the device: %s" % (name, msg)
    assert name not in results, name
    results[name] = [rc, msg]


# ---------------------------------------------------------------------------------------------------- the two *_jobs entry points
def fwd_job(kind, keep):
    q = _abi.FieldJob()
    q.kind, q.n_rays, q.n_samples = kind, 5, 7
    q.origins, q.directions, q.pixel_area, q.euclid_bins, q.sqradius, q.out_rgb = (fake() for _ in range(6))
    fo, fs = filled(_abi.FieldOutputs), filled(_abi.FieldSaved)
    keep += [fo, fs]
    q.out, q.saved = C.pointer(fo), C.pointer(fs)
    return q, {"out": fo, "saved": fs}


def bwd_job(kind, keep):
    q = _abi.FieldBwdJob()
    q.kind, q.n_rays, q.n_samples, q.need_input_grad = kind, 5, 7, 1
    q.origins, q.directions, q.pixel_area, q.euclid_bins, q.sqradius, q.g_rgb = (fake() for _ in range(6))
    st = {"fwd": filled(_abi.FieldOutputs), "saved": filled(_abi.FieldSaved),
          "gin": filled(_abi.FieldGradsIn, ("sigma", "color", "weights")), "gout": filled(_abi.FieldGradsOut)}
    keep += list(st.values())
    q.fwd, q.saved, q.gin, q.gout = (C.pointer(st[k]) for k in ("fwd", "saved", "gin", "gout"))
    return q, st


def job_edits(backward):
    """(label, kinds it applies to, function(job, structs)) + ("soft",) if the edit alone leaves the job valid."""
    def setter(path, value):
        def f(q, st):
            if "." in path:
                s, m = path.split(".")
                setattr(st[s], m, value)
            elif value is None and path in st:
                setattr(q, path, type(getattr(q, path))())  # NULL struct pointer
            else:
                setattr(q, path, value)
        return f

    e = [("kind=2", (0, 1), setter("kind", 2)), ("n_rays=-1", (0, 1), setter("n_rays", -1)), ("n_rays=0", (0, 1), setter("n_rays", 0), "soft"),
         ("n_samples=0", (0,), setter("n_samples", 0)), ("saved=NULL", (0, 1), setter("saved", None))]
    e += [(p + "=NULL", (0,), setter(p, None)) for p in ("origins", "pixel_area", "euclid_bins")]
    e += [("directions=NULL", (0, 1), setter("directions", None)), ("sqradius=NULL", (1,), setter("sqradius", None))]
    if not backward:
        e += [("out=NULL", (0,), setter("out", None)), ("out_rgb=NULL", (1,), setter("out_rgb", None))]
        e += [("saved." + m + "=NULL", (0, 1), setter("saved." + m, None)) for m in SAVED_REQUIRED]

        def all_saved_null(q, st):
            for m, _ in _abi.FieldSaved._fields_:
                setattr(st["saved"], m, None)
        e += [("saved.*=NULL (an eval job)", (0, 1), all_saved_null)]
    else:
        e += [(p + "=NULL", (0,), setter(p, None)) for p in ("fwd", "gin")]
        e += [("gout=NULL", (0, 1), setter("gout", None)), ("g_rgb=NULL", (1,), setter("g_rgb", None))]
        e += [(p + "=NULL", (0, 1), setter(p, None)) for p in ("saved.relu_bits", "saved.heads", "gout.dy")]
        e += [(p + "=NULL", (0, 1), setter(p, None), "soft") for p in ("saved.enc", "gout.d_input")]
        e += [("need_input_grad=0", (0, 1), setter("need_input_grad", 0), "soft")]
        e += [(p + "=NULL", (0,), setter(p, None)) for p in ("fwd.raw_density", "fwd.diff", "fwd.tint")]
        e += [(p + "=NULL", (0,), setter(p, None), "soft") for p in ("gin.weights", "saved.normals", "fwd.pred_normals", "fwd.n_dot_d")]
        e += [(p, (0,), setter(p, 0xABC000), "soft") for p in ("gin.ray_pn_loss", "gin.ray_ori_loss")]
    return e


def run_jobs(lib, results):
    for backward in (False, True):
        fn = "rsn_field_backward_jobs" if backward else "rsn_field_forward_train_jobs"
        make, arr_t = (bwd_job, _abi.FieldBwdJob) if backward else (fwd_job, _abi.FieldJob)
        edits = job_edits(backward)

        def launch(kinds, changes, n_jobs=None, desc="ok", packed="ok", jobs_null=False):
            keep = []
            arr = (arr_t * max(len(kinds), 1))()
            for k, kind in enumerate(kinds):
                q, st = make(kind, keep)
                for change in changes:
                    if change[0] == k:
                        change[3](q, st)
                arr[k] = q
            d = make_desc()
            n = len(kinds) if n_jobs is None else n_jobs
            return lambda lib: getattr(lib, fn)(None if desc is None else C.byref(d), None if packed is None else fake(), n,
                                                None if jobs_null else arr, None)

        record(lib, results, fn + " | desc=NULL", launch((0, 1), [], desc=None))
        record(lib, results, fn + " | jobs=NULL", launch((0, 1), [], jobs_null=True))
        record(lib, results, fn + " | desc=NULL & jobs=NULL", launch((0, 1), [], desc=None, jobs_null=True))
        for n in (0, -1, RSN_MAX_JOBS + 1):
            record(lib, results, fn + " | n_jobs=%d" % n, launch((0, 1), [], n_jobs=n))
        zero = [e for e in edits if e[0] == "n_rays=0"][0][:3]
        for kinds in ((0,), (1,), (0, 1), (1, 0), (0, 0, 1)):
            tag = fn + " | kinds " + "".join(map(str, kinds))
            allzero = [(k, *zero) for k in range(len(kinds))]
            record(lib, results, tag + " | n_rays=0 in every job", launch(kinds, allzero))
            record(lib, results, tag + " | n_rays=0 in every job & packed=NULL", launch(kinds, allzero, packed=None))
            placed = [(k, *e) for k in range(len(kinds)) for e in edits if kinds[k] in e[1]]
            for combo in [(p,) for p in placed] + list(itertools.combinations(placed, 2)):
                if kinds != (0, 1) and len(combo) == 2:
                    continue  # pairs: in the frustum + inf launch (the training step's own)
                # the jobs that are not edited have no rays, and neither have the edited ones when no edit is an error by itself (the
                # zeroing goes last): a launch that the edits do not stop returns RSN_OK without work
                soft = all(len(c) > 4 for c in combo)
                rest = [z for z in allzero if soft or z[0] not in [c[0] for c in combo]]
                label = " & ".join("job %d: %s" % (c[0], c[1]) for c in combo) + (" (no rays)" if soft else "")
                record(lib, results, tag + " | " + label, launch(kinds, list(combo) + rest))


def field_error_matrix(lib):
    results = {}
    run_singles(lib, results)
    run_jobs(lib, results)
    return results


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    res = field_error_matrix(_abi.load_library())
    # {case: index into "answers"}: the few dozen distinct (return code, message) pairs are stored once
    answers = sorted(set(map(tuple, res.values())), key=lambda a: (-a[0], a[1]))
    text = json.dumps({"answers": answers, "cases": {k: answers.index(tuple(v)) for k, v in sorted(res.items())}}, indent=0) + "\n"
    if out == "-":
        sys.stdout.write(text)
    else:
        with open(out, "w") as fh:
            fh.write(text)
        print("%d cases -> %s (library: %s)" % (len(res), out, os.environ.get("RSN_LIBRARY", "the tree's own")), file=sys.stderr)
