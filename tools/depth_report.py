#!/usr/bin/env python3
"""What depth supervision costs and does (trainer --depth-loss, eval --depth; rsn_depth_loss_forward / _backward, rsn_gather_ray_depth,
rsn_depth_error): profiles/depth_loss.json.

    python tools/depth_report.py --parent-tree DIR [--out profiles/depth_loss.json] [--images 24] [--blocks 4] [--steps 10]

Four measurements, all on the GPU (there is no fallback):
  ratios    the four kernels against the float64 references of tests/depth_reference.py on the GPU tests' own inputs, in units of
            2^-24 of the scale (what the RATIO lines of tests/test_depth_gpu.py print), worst over the shapes.
  kernels   rsn_depth_loss_forward and rsn_depth_loss_backward (accumulate = 1) at the headline shape, 4096 rays x 128 samples, on seeded
            densities with a target on four rays of five; rsn_gather_ray_depth for 4096 rays of 24 views of 800 x 800; rsn_depth_error
            on an 800 x 800 view: each call between two HIP events after 3 untimed calls, median of 20.
  step      the headline training step (4096 rays x (128 + 128 + 64 + 64), 8 x 256, exact fp32; next_train + train_step) in child
            processes that each import ONE tree: the parent commit's (DIR: a built checkout of it, which has no such term) and this
            one with the term off, on the fine level, and on both levels, in the order parent / off / fine / both / both / fine / off /
            parent.  The three arms of this tree draw from a scene WITH depth maps (off: trainer.train's rule, the maps are dropped
            before the upload).  FusedRAdam runs with lr = 0: the term changes what the model learns and with it the number of
            reflected rays, which is work of the step that these kernels do not do; with the parameters held every
            arm has the same work.
  toy_scene tests/test_depth_gpu.run_end_to_end: the sphere with analytic depth maps, deterministic steps with and without the term,
            eval --depth on the held-out views.  One run each: it sizes the end-to-end test's bound, it is not a claim."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = {"parent": (None, None), "off": (None, None), "fine": (0.01, None), "both": (0.01, 0.01)}  # (fine, coarse) coefficients


def _args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (the step comparison is skipped without it)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "depth_loss.json"))
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--no-toy-scene", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--arm", default="off", choices=tuple(ARMS), help=argparse.SUPPRESS)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.tree if ARGS.child else HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import ops  # noqa: E402
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager  # noqa: E402

DEV = torch.device("cuda:0")
SIZE, FOCAL = 800, 1111.111  # the Blender scenes: 800 x 800, camera_angle_x 0.6911
COEF = 0.01                  # a starting point; not measured on a scene


def blender_like_scene(n, depths):
    """n views of 800 x 800 RGBA noise from a radius-4 shell looking at the origin (the timing does not depend on the content), with
    z-depth maps on [2, 6] and a fifth of the pixels unmeasured when asked for."""
    rng = np.random.default_rng(0)
    ims = rng.integers(0, 256, size=(n, SIZE, SIZE, 4), dtype=np.uint8)
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
    kw = {}
    if depths:
        d = (2.0 + 4.0 * rng.random((n, SIZE, SIZE), dtype=np.float32))
        d[rng.random((n, SIZE, SIZE), dtype=np.float32) < 0.2] = 0.0
        kw["depths"] = d
    return BlenderScene.from_arrays(ims, np.stack(poses).astype(np.float32), focal=FOCAL, **kw)


def between_events(fn, reps=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


# ------------------------------------------------------------------------------------------------ child: the training step
def child():
    import dataclasses

    from reflect_sampling_nerf_amd.parallel import train_step

    torch.manual_seed(0)
    cfg = pkg.ReflectSamplingNeRFModelConfig()  # the reference defaults: 8 x 256, 128 + 128 + 64 + 64 samples
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 2.0  # bench.py's set-up: a field that is not empty
    model.to(DEV).train()
    model.field.set_mma_mode("f32")
    fine, coarse = ARMS[ARGS.arm]
    for key, coef in (("depth_loss_fine", fine), ("depth_loss_coarse", coarse)):
        if coef is not None:
            model.config.loss_coefficients[key] = coef
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=0.0, eps=1e-15)  # lr = 0: the same work in every arm (see above)
    scene = blender_like_scene(ARGS.images, depths=ARGS.arm != "parent")
    if ARGS.arm == "off":
        scene = dataclasses.replace(scene, depths=None)  # what trainer.train does when no coefficient is set
    dm = RayDataManager(scene, DEV, num_rays_per_batch=4096, seed=0)
    step = [0]

    def one():
        rb, b = dm.next_train(step[0])
        train_step(model, rb, b, opt, None, 100 + step[0])
        step[0] += 1

    for _ in range(ARGS.warmup):
        one()
    torch.cuda.synchronize()
    blocks = [round(between_events(one, ARGS.steps), 4) for _ in range(ARGS.blocks)]
    print("RESULT " + json.dumps({"ms_per_step_blocks": blocks}))


# ------------------------------------------------------------------------------------------------ parent
def _median_us(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = sorted(between_events(call) * 1e3 for _ in range(20))
    return {"median_us": round(statistics.median(t), 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2)}


def kernel_times():
    from reflect_sampling_nerf_amd import metrics

    R, S = 4096, 128
    g = torch.Generator().manual_seed(0)
    sigma = (torch.rand(R, S, generator=g) * 8.0 * (torch.rand(R, S, generator=g) > 0.5)).to(DEV)
    nears, fars = torch.full((R,), 2.0, device=DEV), torch.full((R,), 6.0, device=DEV)
    _, eb = ops.sample_spaced(R, None, S, 0, 1.0, nears, fars, torch.rand(R, S + 1, generator=g).to(DEV))
    target = ((2.2 + 3.6 * torch.rand(R, generator=g)) * (torch.rand(R, generator=g) > 0.2)).to(DEV)
    g_ray = torch.full((R,), COEF / R, device=DEV)
    g_sigma = torch.zeros(R, S, device=DEV)
    scene = blender_like_scene(24, depths=True)
    dm = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=0)
    _, batch = dm.next_train(0)
    view_t = dm.view_ray_depth(0)
    view_d = view_t + 0.1
    out = {"shape": {"rays": R, "samples": S, "views": [24, SIZE, SIZE]}, "method": "one call between two HIP events, median of 20 after 3 untimed",
           "rsn_depth_loss_forward": _median_us(lambda: ops.depth_loss_forward(R, None, S, eb, sigma, target, 0.1)),
           "rsn_depth_loss_backward": _median_us(lambda: ops.depth_loss_backward(R, None, S, eb, sigma, target, 0.1, g_ray, g_sigma, accumulate=True)),
           "rsn_gather_ray_depth_4096_rays": _median_us(lambda: dm.ray_depth(batch["indices"])),
           "rsn_depth_error_800x800": _median_us(lambda: metrics.depth_error(view_d, view_t))}
    return out


def ratios():
    """The GPU tests' own cases and checks, their WORST table read afterwards."""
    from tests import render_reference as rr
    from tests import test_depth_gpu as t

    for S in t.S_CASES:
        case = t._case(t.R_CASE, S, DEV)
        t._check_both(f"S{S}", case, t._forward(case, t.R_CASE, S), t._backward(case, t.R_CASE, S, 0))
    case = t._case(rr.BIG_R, rr.BIG_S, DEV)
    t._check_both("grid stride", case, t._forward(case, rr.BIG_R, rr.BIG_S), t._backward(case, rr.BIG_R, rr.BIG_S, 0))
    worst_gather = 0.0
    for name, table in t.GATHER_TABLES.items():
        depths, idx, level, cams = t._gather_inputs(table)
        k = (61.0, 64.5, t.GW / 2 - 0.7, t.GH / 2 + 0.4)
        got = t._gather(depths, idx, None, cams, k, False, False, DEV)
        want = t.dz.ray_depth_reference(idx, None, depths, cams, k, False)
        live = want != 0
        worst_gather = max(worst_gather, float((np.abs(got - want)[live] / want[live]).max()) / 2.0 ** -24)
    return {"unit": "2^-24 of the scale (tests/test_depth_gpu.py)", "bound": t.BOUND, "loss_ray": round(t.WORST["loss_ray"], 3),
            "g_sigma": round(t.WORST["g_sigma"], 3), "gather_ray_depth_relative": round(worst_gather, 3), "gather_bound": 2.0}


def step_times():
    parent = os.path.abspath(ARGS.parent_tree)
    order = ["parent", "off", "fine", "both", "both", "fine", "off", "parent"]
    runs = []
    for arm in order:
        tree = parent if arm == "parent" else HERE
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--arm", arm, "--images", str(ARGS.images),
               "--blocks", str(ARGS.blocks), "--steps", str(ARGS.steps), "--warmup", str(ARGS.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=tree)
        if res.returncode != 0:
            raise RuntimeError(f"{arm}: child exited with {res.returncode}\n{res.stderr[-2000:]}")
        line = [s for s in res.stdout.splitlines() if s.startswith("RESULT ")][-1]
        runs.append({"arm": arm, **json.loads(line[7:])})
        print(arm, runs[-1]["ms_per_step_blocks"], flush=True)
    blocks = {a: [t for r in runs if r["arm"] == a for t in r["ms_per_step_blocks"]] for a in ARMS}
    med = {a: statistics.median(v) for a, v in blocks.items()}
    return {"shape": {"rays": 4096, "samples": [128, 128, 64, 64], "layers": 8, "width": 256, "mma": "f32", "images": ARGS.images, "size": [SIZE, SIZE]},
            "coefficient": COEF,
            "method": f"one process per run (a process binds one build), order {' / '.join(order)}; per run {ARGS.warmup} untimed steps, then "
                      f"{ARGS.blocks} blocks of {ARGS.steps} steps (next_train + train_step), each block between two HIP events; FusedRAdam with lr = 0 (the same work in every arm)",
            "runs": runs, "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
            "spread_ms": {a: round(max(v) - min(v), 4) for a, v in blocks.items()},
            "minus_parent_ms": {a: round(med[a] - med["parent"], 4) for a in ("off", "fine", "both")},
            "minus_off_ms": {a: round(med[a] - med["off"], 4) for a in ("fine", "both")}}


def toy_scene(tmp):
    from tests import test_depth_gpu as t

    arms = t.run_end_to_end(tmp)
    return {"scene": "Lambert sphere with analytic z-depth maps, 24 train / 4 test views of 48 x 48; 4 x 64 field, 32 + 32 + 16 + 16 samples",
            "steps": t.E2E_STEPS, "rays": 1024, "deterministic": True, "coefficient": t.E2E_COEF, "depth_sigma": t.E2E_SIGMA,
            "off": arms["off"], "on": arms["on"], "note": "one run each on a toy scene: it sizes the end-to-end test's bound, it is not a claim"}


def main():
    import tempfile

    assert torch.cuda.is_available(), "tools/depth_report.py needs a GPU"
    pkg.load_library()
    report = {"tool": "tools/depth_report.py", "device": torch.cuda.get_device_name(0)}
    report["ratios"] = ratios()
    print("ratios", json.dumps(report["ratios"]), flush=True)
    report["kernels"] = kernel_times()
    print("kernels", json.dumps(report["kernels"]), flush=True)
    if ARGS.parent_tree:
        report["step"] = step_times()
        print("step", json.dumps(report["step"]["ms_per_step_median"]), json.dumps(report["step"]["spread_ms"]), flush=True)
    if not ARGS.no_toy_scene:
        with tempfile.TemporaryDirectory() as tmp:
            report["toy_scene"] = toy_scene(tmp)
        print("toy_scene", json.dumps(report["toy_scene"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    child() if ARGS.child else main()
