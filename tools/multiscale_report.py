#!/usr/bin/env python3
"""What multi-scale training and evaluation cost and give (RayDataManager levels, trainer --multiscale): profiles/multiscale.json.

    python tools/multiscale_report.py --parent-tree DIR [--out profiles/multiscale.json] [--images 100] [--blocks 4] [--steps 10]

Four measurements, all on the GPU (there is no fallback):
  pyramid   rsn_build_pyramid for --images images of 800 x 800 with L = 2 .. 5 (the headline: L = 4), each call between two HIP
            events after 3 untimed calls, median of 20; and the same call on ONE 16 x 16 image, which is the cost of a launch.
  sampler   rsn_sample_pyramid_rays (L = 4) against rsn_sample_camera_rays at R = 4096 on the same scene: blocks of 200 launches
            between two events, the two calls alternating, 6 blocks each after 2 untimed ones; us per launch.
  step      the headline training step (4096 rays x (128 + 128 + 64 + 64), 8 x 256, exact fp32; next_train + train_step) on that
            scene, in child processes that each import ONE tree: the parent commit's (DIR: a built checkout of it, single-scale) and
            this one with levels = 4, in the order parent / this / this / parent.  A child runs 40 untimed steps, then --blocks blocks
            of --steps steps, each block between two HIP events.  A process binds one build of the library, so the arms alternate
            per process and not per block.
  toy_scene test-view PSNR per scale on the Lambert sphere of tests/test_pyramid_gpu.py after 400 steps with multiscale 3 and after
            400 single-scale steps, both scored at the three scales, beside the untrained model: one run each, a record, not a claim."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (the step comparison is skipped without it)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "multiscale.json"))
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--no-toy-scene", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--levels", type=int, default=1, help=argparse.SUPPRESS)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.tree if ARGS.child else HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import _abi  # noqa: E402
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager  # noqa: E402

DEV = torch.device("cuda:0")
SIZE, FOCAL = 800, 1111.111  # the Blender scenes: 800 x 800, camera_angle_x 0.6911


def blender_like_scene(n):
    """n views of 800 x 800 RGBA noise from a radius-4 shell looking at the origin (the timing does not depend on the content)."""
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
    return BlenderScene.from_arrays(ims, np.stack(poses).astype(np.float32), focal=FOCAL)


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
    from reflect_sampling_nerf_amd.parallel import train_step

    torch.manual_seed(0)
    cfg = pkg.ReflectSamplingNeRFModelConfig()  # the reference defaults: 8 x 256, 128 + 128 + 64 + 64 samples
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 2.0  # bench.py's set-up: a field that is not empty
    model.to(DEV).train()
    model.field.set_mma_mode("f32")
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)
    extra = {"levels": ARGS.levels} if ARGS.levels > 1 else {}  # the parent's data manager has no such argument
    dm = RayDataManager(blender_like_scene(ARGS.images), DEV, num_rays_per_batch=4096, seed=0, **extra)
    step = [0]

    def one():
        rb, b = dm.next_train(step[0])
        train_step(model, rb, b, opt, None, 100 + step[0])
        step[0] += 1

    for _ in range(ARGS.warmup):
        one()
    torch.cuda.synchronize()
    blocks = [round(between_events(one, ARGS.steps), 4) for _ in range(ARGS.blocks)]
    print("RESULT " + json.dumps({"levels": ARGS.levels, "ms_per_step_blocks": blocks}))


# ------------------------------------------------------------------------------------------------ parent
def pyramid_times(lib, scene):
    dm = RayDataManager(scene, DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    out = {"images": scene.num_images, "size": [SIZE, SIZE], "method": "one call between two HIP events, median of 20 after 3 untimed", "levels": {}}

    def timed(n, h, w, levels, images):
        from reflect_sampling_nerf_amd.data import pyramid_layout

        pixels = pyramid_layout(n, h, w, levels)[1][-1]
        pyr = torch.empty(pixels, 3, device=DEV)
        call = lambda: _abi.check(lib.rsn_build_pyramid(n, h, w, levels, _abi.ptr(images), _abi.ptr(pyr), pixels, stream))  # noqa: E731
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        t = sorted(between_events(call) for _ in range(20))
        return {"median_ms": round(statistics.median(t), 4), "min_ms": round(t[0], 4), "max_ms": round(t[-1], 4), "pixels_written": pixels,
                "bytes_read_min": n * h * w * 4 * (levels - 1), "bytes_written": pixels * 12}

    for levels in (2, 3, 4, 5):
        out["levels"][str(levels)] = timed(scene.num_images, SIZE, SIZE, levels, dm.images)
    tiny = torch.zeros(1, 16, 16, 4, dtype=torch.uint8, device=DEV)
    out["one_16x16_image_levels_4"] = timed(1, 16, 16, 4, tiny)
    r = out["levels"]["4"]
    r["tb_per_s_of_min_traffic"] = round((r["bytes_read_min"] + r["bytes_written"]) / (r["median_ms"] * 1e-3) / 1e12, 3)
    return out


def sampler_times(scene):
    R, reps = 4096, 200
    single = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=0)
    multi = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=0, levels=4)
    step = [0]

    def run(dm):
        def fn():
            dm.next_train(step[0])
            step[0] += 1
        return fn

    arms = {"rsn_sample_camera_rays": run(single), "rsn_sample_pyramid_rays_levels_4": run(multi)}
    blocks = {k: [] for k in arms}
    for rep in range(8):
        for k, fn in arms.items():
            t = between_events(fn, reps) * 1e3
            if rep >= 2:
                blocks[k].append(round(t, 3))
    return {"rays": R, "method": f"next_train (two allocations + the launch) {reps} times between two HIP events, arms alternating, 6 blocks each "
                                 "after 2 untimed; the figures are us per call of a back-to-back stream, not a kernel's own time",
            "us_per_call_blocks": blocks, "us_per_call_median": {k: round(statistics.median(v), 3) for k, v in blocks.items()}}


def step_times():
    parent = os.path.abspath(ARGS.parent_tree)
    order = [("parent", parent, 1), ("this_levels_4", HERE, 4), ("this_levels_4", HERE, 4), ("parent", parent, 1)]
    runs = []
    for name, tree, levels in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--levels", str(levels), "--images", str(ARGS.images),
               "--blocks", str(ARGS.blocks), "--steps", str(ARGS.steps), "--warmup", str(ARGS.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=tree)
        if res.returncode != 0:
            raise RuntimeError(f"{name}: child exited with {res.returncode}\n{res.stderr[-2000:]}")
        line = [s for s in res.stdout.splitlines() if s.startswith("RESULT ")][-1]
        runs.append({"arm": name, **json.loads(line[7:])})
        print(name, runs[-1]["ms_per_step_blocks"], flush=True)
    med = {a: statistics.median([t for r in runs if r["arm"] == a for t in r["ms_per_step_blocks"]]) for a in ("parent", "this_levels_4")}
    per_run = [statistics.median(r["ms_per_step_blocks"]) for r in runs]
    return {"shape": {"rays": 4096, "samples": [128, 128, 64, 64], "layers": 8, "width": 256, "mma": "f32", "images": ARGS.images, "size": [SIZE, SIZE]},
            "method": f"one process per run (a process binds one build), order parent / this / this / parent; per run {ARGS.warmup} untimed steps, then "
                      f"{ARGS.blocks} blocks of {ARGS.steps} steps (next_train + train_step), each block between two HIP events",
            "runs": runs, "ms_per_step_median": {k: round(v, 4) for k, v in med.items()},
            "this_minus_parent_ms": round(med["this_levels_4"] - med["parent"], 4),
            "paired_run_differences_ms": [round(per_run[1] - per_run[0], 4), round(per_run[2] - per_run[3], 4)],
            "spread_ms": {a: round(max(t for r in runs if r["arm"] == a for t in r["ms_per_step_blocks"]) -
                                   min(t for r in runs if r["arm"] == a for t in r["ms_per_step_blocks"]), 4) for a in med}}


def toy_scene(tmp):
    from reflect_sampling_nerf_amd import trainer
    from tests.test_pyramid_gpu import E2E_STEPS, _cfg, _sphere_scene, _untrained_checkpoint

    train_scene, test_scene = _sphere_scene(24), _sphere_scene(4, offset=0.37)
    kw = dict(steps=E2E_STEPS, rays=1024, save_every=0, log_every=0, seed=0, device=DEV, model_config=_cfg(), log=None)
    cks = {"untrained": _untrained_checkpoint(os.path.join(tmp, "init")),
           "multiscale_3": trainer.train(train_scene, os.path.join(tmp, "multi"), multiscale=3, **kw),
           "single_scale": trainer.train(train_scene, os.path.join(tmp, "single"), **kw)}
    out = {"scene": "Lambert sphere, 24 train / 4 test views of 48 x 48; 4 x 64 field, 32 + 32 + 16 + 16 samples", "steps": E2E_STEPS, "rays": 1024,
           "note": "one run each on a toy scene: a record, not a claim"}
    for name, ck in cks.items():
        r = trainer.evaluate(test_scene, ck, device=DEV, model_config=_cfg(), multiscale=3)["results"]
        out[name] = {k: round(r[k], 4) for k in sorted(r) if k.startswith(("psnr", "fine_ssim")) and not k.endswith("_std")}
    for name in ("multiscale_3", "single_scale"):
        out[name + "_psnr_gain_db"] = {f"x{s}": round(out[name][f"psnr_x{s}"] - out["untrained"][f"psnr_x{s}"], 4) for s in (1, 2, 4)}
    return out


def main():
    import tempfile

    assert torch.cuda.is_available(), "tools/multiscale_report.py needs a GPU"
    lib = pkg.load_library()
    scene = blender_like_scene(ARGS.images)
    report = {"tool": "tools/multiscale_report.py", "device": torch.cuda.get_device_name(0)}
    report["pyramid"] = pyramid_times(lib, scene)
    print("pyramid", json.dumps(report["pyramid"]["levels"]), flush=True)
    report["sampler"] = sampler_times(scene)
    print("sampler", report["sampler"]["us_per_call_median"], flush=True)
    del scene
    torch.cuda.empty_cache()
    if ARGS.parent_tree:
        report["step"] = step_times()
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
