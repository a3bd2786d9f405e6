#!/usr/bin/env python3
"""What the opt-in geometry metrics of `eval --normals` cost and say (metrics.normal_error; rsn_normal_error): profiles/geometry_metrics.json.

    python tools/geometry_report.py [--parent-tree DIR] [--out profiles/geometry_metrics.json] [--views 4] [--size 200] [--repeats 3]

Four measurements, all on the GPU (there is no fallback):
  kernel_vs_fp64  the worst |error_map - float64 reference| in degrees over the sizes and seeded inputs of tests/test_geometry_gpu.py
                  (tests.test_geometry_gpu.worst_map_error), unrotated and rotated: the source of that file's tolerance.
  kernel          rsn_normal_error (both launches, with accumulation and error map) on an 800 x 800 view: 50 calls between two HIP
                  events after 10 untimed, the median of 20 such windows; the 27 bytes a pixel the call has to move over that time, and
                  over the chip's peak rate.  The 17 MB of a view stay in the last-level cache between calls: a warm figure.
  eval            trainer.evaluate on --views noise views of --size x --size (the reference model, 8 x 256, 128 + 128 + 64 + 64 samples,
                  untrained) in child processes that each import ONE tree: the parent commit's (--parent-tree: a built checkout of it,
                  which has no such metric), this one without normals and this one with, in the order parent / off / on / on / off /
                  parent.  A child runs one untimed evaluate, then --repeats timed ones (host clock around the call, which ends in
                  device-to-host reads of every view's metrics); per view = the call's time over its views, checkpoint load included.
  toy_scene       the Lambert sphere of the tests with analytic world-space normal maps (24 train / 4 test views of 48 x 48): normal_mae
                  and alpha_mae of the untrained model and after 400 deterministic steps with --distortion-loss 0.01 and without.  One
                  run each: a record, not a claim.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("parent", "off", "on")


def _args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (its arm of the eval comparison is skipped without it)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "geometry_metrics.json"))
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-toy-scene", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--arm", default="off", choices=ARMS, help=argparse.SUPPRESS)
    ap.add_argument("--ckpt", default=None, help=argparse.SUPPRESS)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.tree if ARGS.child else HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import trainer  # noqa: E402
from reflect_sampling_nerf_amd.data import BlenderScene  # noqa: E402

DEV = torch.device("cuda:0")
HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X HBM3E, specification
BYTES_PER_PIXEL = 27           # 12 prediction + 4 accumulation + 3 normal bytes + 4 RGBA (the alpha's pixel) + 4 error map
DISTORTION = 0.01              # mip-NeRF 360's coefficient; not measured on this method


def noise_scene(n, size, normals):
    """n views of size x size RGBA noise (and noise normal maps) from a radius-4 shell looking at the origin: the time does not depend
    on the content."""
    rng = np.random.default_rng(0)
    ims = rng.integers(0, 256, size=(n, size, size, 4), dtype=np.uint8)
    nrm = rng.integers(0, 256, size=(n, size, size, 3), dtype=np.uint8)
    k = np.arange(n) + 0.5
    z = 0.8 * (1 - 2 * k / (n + 1))
    phi = k * np.pi * (3 - np.sqrt(5))
    pos = 4.0 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1)
    poses = []
    for p in pos:
        back = p / np.linalg.norm(p)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        poses.append(np.concatenate([np.stack([right, np.cross(back, right), back], 1), p[:, None]], 1))
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    extra = {"normals": nrm} if normals else {}
    return BlenderScene.from_arrays(ims, np.stack(poses).astype(np.float32), focal=focal, **extra)


# ------------------------------------------------------------------------------------------------ child: evaluate in one tree
def child():
    on = ARGS.arm == "on"
    scene = noise_scene(ARGS.views, ARGS.size, normals=on)
    extra = {"normals": True} if on else {}
    times = []
    for rep in range(ARGS.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = trainer.evaluate(scene, ARGS.ckpt, device=DEV, **extra)
        torch.cuda.synchronize()
        if rep:
            times.append(round((time.perf_counter() - t0) / scene.num_images * 1e3, 3))
    print("RESULT " + json.dumps({"ms_per_view": times, "keys": sorted(res["results"])}))


# ------------------------------------------------------------------------------------------------ parent
def kernel_vs_fp64():
    from tests import geometry_reference as ref
    from tests.test_geometry_gpu import SIZES, worst_map_error

    plain, where = worst_map_error()
    rotated, where_r = worst_map_error(rotation=ref.rotation_matrix())
    return {"sizes": list(SIZES), "seed": 0, "inputs": "tests.geometry_reference.kernel_inputs",
            "worst_abs_deg": float(f"{plain:.4g}"), "at": where, "worst_abs_deg_rotated": float(f"{rotated:.4g}"), "at_rotated": where_r,
            "note": "tests/test_geometry_gpu.py bounds the per-pixel error by four times worst_abs_deg"}


def kernel_time():
    from reflect_sampling_nerf_amd import metrics
    from tests import geometry_reference as ref

    H = W = 800
    normals, acc, gt, rgba = ref.kernel_inputs(H * W, seed=2)
    n, a = torch.from_numpy(normals).to(DEV).view(H, W, 3), torch.from_numpy(acc).to(DEV).view(H, W, 1)
    g, r = torch.from_numpy(gt).to(DEV).view(H, W, 3), torch.from_numpy(rgba).to(DEV).view(H, W, 4)
    lib = pkg.load_library()
    from reflect_sampling_nerf_amd import _abi

    emap = torch.empty(H, W, device=DEV)
    nbytes = int(lib.rsn_normal_error_workspace_bytes(H * W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(4, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call():
        _abi.check(lib.rsn_normal_error(H * W, _abi.ptr(n), _abi.ptr(a), _abi.ptr(g), _abi.ptr(r), None, _abi.ptr(emap), _abi.ptr(ws), nbytes,
                                        _abi.ptr(out), stream))

    for _ in range(10):
        call()
    torch.cuda.synchronize()
    windows, per = [], 50
    for _ in range(20):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(per):
            call()
        e.record()
        e.synchronize()
        windows.append(s.elapsed_time(e) / per * 1e3)
    windows.sort()
    med = statistics.median(windows)
    nbytes_moved = BYTES_PER_PIXEL * H * W
    check = metrics.normal_error(n, a, g, r)
    return {"shape": [H, W], "method": f"{per} calls (two launches each) between two HIP events after 10 untimed, median of 20 windows; inputs cache-warm",
            "median_us": round(med, 2), "min_us": round(windows[0], 2), "max_us": round(windows[-1], 2),
            "bytes": nbytes_moved, "bytes_per_pixel": BYTES_PER_PIXEL, "achieved_gb_per_s": round(nbytes_moved / (med * 1e-6) / 1e9, 1),
            "time_at_hbm_peak_us": round(nbytes_moved / HBM_PEAK_BYTES_PER_S * 1e6, 2),
            "share_of_hbm_peak": round(nbytes_moved / HBM_PEAK_BYTES_PER_S / (med * 1e-6), 4),
            "bound": "bytes over the peak HBM rate: the call does no arithmetic to speak of.  The launch is at most 256 workgroups of 256 lanes",
            "normal_mae_of_the_inputs": float(check["normal_mae"])}


def eval_times(tmp):
    model = trainer.make_model(None, seed=0)
    opt0 = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ck = trainer.save_checkpoint(trainer.checkpoint_path(os.path.join(tmp, "init"), 0), model, opt0, 0)
    del model, opt0
    parent = os.path.abspath(ARGS.parent_tree) if ARGS.parent_tree else None
    order = ["parent", "off", "on", "on", "off", "parent"] if parent else ["off", "on", "on", "off"]
    runs = []
    for arm in order:
        tree = parent if arm == "parent" else HERE
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--arm", arm, "--ckpt", ck, "--views", str(ARGS.views),
               "--size", str(ARGS.size), "--repeats", str(ARGS.repeats)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=tree)
        if res.returncode != 0:
            raise RuntimeError(f"{arm}: child exited with {res.returncode}\n{res.stderr[-2000:]}")
        line = [s for s in res.stdout.splitlines() if s.startswith("RESULT ")][-1]
        runs.append({"arm": arm, **json.loads(line[7:])})
        print(arm, runs[-1]["ms_per_view"], flush=True)
    arms = [a for a in ARMS if a in order]
    every = {a: [t for r in runs if r["arm"] == a for t in r["ms_per_view"]] for a in arms}
    med = {a: statistics.median(v) for a, v in every.items()}
    out = {"shape": {"views": ARGS.views, "size": [ARGS.size, ARGS.size], "layers": 8, "width": 256, "samples": [128, 128, 64, 64], "chunk": trainer.EVAL_CHUNK},
           "method": f"one process per run (a process binds one build), order {' / '.join(order)}; per run one untimed evaluate, then {ARGS.repeats} "
                     "timed ones, host clock around the call; per view = the call over its views, checkpoint load included",
           "runs": [{k: v for k, v in r.items() if k != "keys"} for r in runs],
           "ms_per_view_median": {a: round(v, 3) for a, v in med.items()},
           "spread_ms": {a: round(max(v) - min(v), 3) for a, v in every.items()},
           "on_minus_off_ms": round(med["on"] - med["off"], 3)}
    if parent:
        out["off_minus_parent_ms"] = round(med["off"] - med["parent"], 3)
        keys = {a: next(r["keys"] for r in runs if r["arm"] == a) for a in arms}
        out["off_keys_equal_parent_keys"] = keys["off"] == keys["parent"]
    return out


def toy_scene(tmp):
    from tests.test_geometry_gpu import _cfg, sphere_scene, untrained_checkpoint

    steps = 400
    train_scene, test_scene = sphere_scene(24, normals=False), sphere_scene(4, offset=0.37)
    kw = dict(steps=steps, rays=1024, save_every=0, log_every=0, seed=0, device=DEV, log=None, deterministic=True)
    cks = {"untrained": untrained_checkpoint(os.path.join(tmp, "toy_init")),
           "without": trainer.train(train_scene, os.path.join(tmp, "off"), model_config=_cfg(), **kw),
           "distortion_loss_0.01": trainer.train(train_scene, os.path.join(tmp, "on"), model_config=_cfg(), distortion_loss=DISTORTION, **kw)}
    out = {"scene": "Lambert sphere with analytic world-space normal maps, 24 train / 4 test views of 48 x 48; 4 x 64 field, 32 + 32 + 16 + 16 samples",
           "steps": steps, "rays": 1024, "deterministic": True, "coefficient": DISTORTION,
           "note": "one run each on a toy scene: a record, not a claim"}
    for name, ck in cks.items():
        r = trainer.evaluate(test_scene, ck, device=DEV, model_config=_cfg(), normals=True)["results"]
        out[name] = {k: round(r[k], 4) for k in ("normal_mae", "normal_mae_std", "alpha_mae", "psnr", "fine_ssim")}
        out[name]["normal_mae_views"] = r["normal_mae_views"]
    return out


def main():
    import tempfile

    assert torch.cuda.is_available(), "tools/geometry_report.py needs a GPU"
    pkg.load_library()
    report = {"tool": "tools/geometry_report.py", "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)

    def section(name, fn, *a):  # the file is rewritten after every section: a later failure keeps the earlier ones
        report[name] = fn(*a)
        print(name, json.dumps({k: v for k, v in report[name].items() if k != "runs"}), flush=True)
        with open(ARGS.out, "w") as fh:
            json.dump(report, fh, indent=1)

    section("kernel_vs_fp64", kernel_vs_fp64)
    section("kernel", kernel_time)
    with tempfile.TemporaryDirectory() as tmp:
        if not ARGS.no_toy_scene:
            section("toy_scene", toy_scene, tmp)
        section("eval", eval_times, tmp)
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    child() if ARGS.child else main()
