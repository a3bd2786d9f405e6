#!/usr/bin/env python3
"""What the capture data path costs and how exact it is (rsn_sample_capture_rays / rsn_capture_rays_image): profiles/capture_rays.json.

    python tools/capture_report.py --parent-tree DIR [--out profiles/capture_rays.json] [--images 100] [--blocks 3] [--steps 10]

Four measurements, all on the GPU (there is no fallback):
  accuracy  tests/test_capture_gpu.measure_against_float64: every pixel of every camera of the tests' tables at levels 0 and 1, the
            kernel's error as a share of the tests' bound (4 x the error of the float32 restatement of the recipe).
  sampler   one training batch of 4096 rays from --images images of 800 x 800: rsn_sample_camera_rays of the parent commit's build
            (DIR: a built checkout of it) against rsn_sample_capture_rays of this one with an all-zero-coefficient table and with a
            distorted one.  Child processes that each import ONE tree, in the order parent / zero / distorted / distorted / zero /
            parent; per child 20 untimed calls, then 20 blocks of 50 calls, each block between two HIP events.
  step      the headline training step (4096 rays x (128 + 128 + 64 + 64), 8 x 256, exact fp32; next_train + train_step, FusedRAdam
            with lr = 0 so that every arm does the same work) fed by each of the three samplers, in the same children: --warmup untimed
            steps, then --blocks blocks of --steps steps.
  toy_scene the bound of the end-to-end test: the gain in test-view PSNR of the existing Blender-format path on the PARENT commit
            for the tests' Lambert sphere at the capture test's scale (pinhole cameras, translations times 0.25, collider 0.5 .. 1.5,
            400 steps of the 4 x 64 config), and the gain the capture test itself prints.  One run each: a record, not a claim."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("parent", "zero", "distorted", "blender_gain")


def _args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (only the accuracy is measured without it)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "capture_rays.json"))
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-toy-scene", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--arm", default="zero", choices=ARMS, help=argparse.SUPPRESS)
    return ap.parse_args()


ARGS = _args()
sys.path.insert(0, os.path.abspath(ARGS.tree if ARGS.child else HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager  # noqa: E402

DEV = torch.device("cuda:0")
SIZE, FOCAL = 800, 1111.111  # the Blender scenes: 800 x 800, camera_angle_x 0.6911
COEFFS = (-0.12, 0.03, -0.004, 0.002, -0.0015)  # the tests' k1 k2 k3 p1 p2


def shell(n, radius=4.0, offset=0.0):
    k = np.arange(n) + 0.5 + offset
    z = np.clip(0.8 * (1 - 2 * k / (n + 1)), -0.8, 0.8)
    phi = k * np.pi * (3 - np.sqrt(5))
    poses = []
    for p in radius * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1):
        back = p / np.linalg.norm(p)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        poses.append(np.concatenate([np.stack([right, np.cross(back, right), back], 1), p[:, None]], 1))
    return np.stack(poses).astype(np.float32)


def between_events(fn, reps=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


# ------------------------------------------------------------------------------------------------ children
def child_timing():
    from reflect_sampling_nerf_amd.parallel import train_step

    n = ARGS.images
    ims = np.random.default_rng(0).integers(0, 256, size=(n, SIZE, SIZE, 4), dtype=np.uint8)
    scene = BlenderScene.from_arrays(ims, shell(n), focal=FOCAL)
    if ARGS.arm != "parent":
        row = np.float32([FOCAL, FOCAL, SIZE / 2, SIZE / 2, *(COEFFS if ARGS.arm == "distorted" else (0.0,) * 5)])
        scene.cameras = np.tile(row, (n, 1))
    dm = RayDataManager(scene, DEV, num_rays_per_batch=4096, seed=0)
    step = [0]

    def sample():
        dm.next_train(step[0])
        step[0] += 1

    for _ in range(20):
        sample()
    torch.cuda.synchronize()
    sampler_us = [round(between_events(sample, 50) * 1e3, 3) for _ in range(20)]
    torch.manual_seed(0)
    model = pkg.ReflectSamplingNeRFModelConfig().setup(scene_box=None, num_train_data=1)  # the reference defaults: 8 x 256, 128 + 128 + 64 + 64
    with torch.no_grad():
        model.field.field_output_density.net.bias += 2.0  # bench.py's set-up: a field that is not empty
    model.to(DEV).train()
    model.field.set_mma_mode("f32")
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=0.0, eps=1e-15)  # lr = 0: the same work in every arm and block

    def one():
        rb, b = dm.next_train(step[0])
        train_step(model, rb, b, opt, None, 100 + step[0])
        step[0] += 1

    for _ in range(ARGS.warmup):
        one()
    torch.cuda.synchronize()
    blocks = [round(between_events(one, ARGS.steps), 4) for _ in range(ARGS.blocks)]
    print("RESULT " + json.dumps({"sampler_us_blocks": sampler_us, "ms_per_step_blocks": blocks}))


def child_blender_gain():
    """The tests' Lambert sphere (tests/test_data_gpu._sphere_scene) through the tree's own Blender-format path, at the capture test's
    scale: translations times 0.25, collider 0.5 .. 1.5."""
    import tempfile

    from reflect_sampling_nerf_amd import trainer
    from tests.test_data_gpu import E2E_STEPS, _sphere_scene

    def cfg():
        return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                                  num_reflect_importance_samples=16, base_mlp_num_layers=4, base_mlp_layer_width=64,
                                                  collider_params={"near_plane": 0.5, "far_plane": 1.5})

    train_scene, test_scene = _sphere_scene(24), _sphere_scene(4, offset=0.37)
    for s in (train_scene, test_scene):
        s.c2w[:, :, 3] *= np.float32(0.25)  # BlenderDataParser scale_factor 0.25
    with tempfile.TemporaryDirectory() as tmp:
        init = trainer.make_model(cfg(), seed=0)
        opt0 = pkg.FusedRAdam(init.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
        ck0 = trainer.save_checkpoint(trainer.checkpoint_path(os.path.join(tmp, "init"), 0), init, opt0, 0)
        ck = trainer.train(train_scene, os.path.join(tmp, "run"), steps=E2E_STEPS, rays=1024, save_every=0, log_every=0, seed=0, device=DEV,
                           model_config=cfg(), log=None)
        before = trainer.evaluate(test_scene, ck0, device=DEV, model_config=cfg())["results"]["psnr"]
        after = trainer.evaluate(test_scene, ck, device=DEV, model_config=cfg())["results"]["psnr"]
    print("RESULT " + json.dumps({"steps": E2E_STEPS, "psnr_before": round(before, 4), "psnr_after": round(after, 4), "gain_db": round(after - before, 4)}))


# ------------------------------------------------------------------------------------------------ parent
def run_child(arm, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--arm", arm, "--images", str(ARGS.images),
           "--blocks", str(ARGS.blocks), "--steps", str(ARGS.steps), "--warmup", str(ARGS.warmup)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=tree)
    if res.returncode != 0:
        raise RuntimeError(f"{arm}: child exited with {res.returncode}\n{res.stderr[-2000:]}")
    return json.loads([s for s in res.stdout.splitlines() if s.startswith("RESULT ")][-1][7:])


def timings():
    parent = os.path.abspath(ARGS.parent_tree)
    order = ["parent", "zero", "distorted", "distorted", "zero", "parent"]
    runs = []
    for arm in order:
        runs.append({"arm": arm, **run_child(arm, parent if arm == "parent" else HERE)})
        print(arm, statistics.median(runs[-1]["sampler_us_blocks"]), runs[-1]["ms_per_step_blocks"], flush=True)
    out = {"shape": {"rays": 4096, "images": ARGS.images, "size": [SIZE, SIZE], "samples": [128, 128, 64, 64], "layers": 8, "width": 256, "mma": "f32"},
           "arms": {"parent": "the parent commit's build and package: rsn_sample_camera_rays",
                    "zero": "rsn_sample_capture_rays, a table of equal rows with all-zero coefficients (the pinhole function)",
                    "distorted": f"rsn_sample_capture_rays, every row with (k1, k2, k3, p1, p2) = {COEFFS}: three fp64 solves per ray"},
           "method": f"one process per run (a process binds one build), order {' / '.join(order)}; sampler: 20 untimed calls of next_train, then 20 "
                     f"blocks of 50 calls between two HIP events; step: {ARGS.warmup} untimed steps, then {ARGS.blocks} blocks of {ARGS.steps} steps "
                     "(next_train + train_step) between two HIP events, FusedRAdam with lr = 0",
           "runs": runs}
    for key, name, digits in (("sampler_us_blocks", "sampler_us", 3), ("ms_per_step_blocks", "ms_per_step", 4)):
        blocks = {a: [t for r in runs if r["arm"] == a for t in r[key]] for a in order[:3]}
        med = {a: statistics.median(v) for a, v in blocks.items()}
        out[name] = {"median": {a: round(v, digits) for a, v in med.items()},
                     "spread": {a: round(max(v) - min(v), digits) for a, v in blocks.items()},
                     "per_run_median": {a: [round(statistics.median(r[key]), digits) for r in runs if r["arm"] == a] for a in order[:3]},
                     "minus_parent": {a: round(med[a] - med["parent"], digits) for a in ("zero", "distorted")}}
    return out


def toy_scene():
    out = {"scene": "Lambert sphere of radius 0.8 seen from a radius-4 shell, 48 x 48 views; 4 x 64 field, 32 + 32 + 16 + 16 samples; 400 steps of 1024 rays",
           "blender_path_on_parent": {"what": "24 train / 4 test pinhole views, translations times 0.25 (scale_factor 0.25), collider 0.5 .. 1.5",
                                      **run_child("blender_gain", os.path.abspath(ARGS.parent_tree))},
           "note": "one run each on a toy scene: a record, not a claim"}
    res = subprocess.run([sys.executable, "-m", "pytest", "tests/test_capture_gpu.py", "-q", "-s", "-k", "test_train_eval_render_end_to_end"],
                         capture_output=True, text=True, timeout=280, cwd=HERE)
    m = re.search(r"capture end to end: held-out psnr ([-\d.]+) -> ([-\d.]+) dB \(gain ([-\d.]+)\)", res.stdout)
    if m is None:
        raise RuntimeError("the capture end-to-end test printed no result\n" + res.stdout[-2000:] + res.stderr[-2000:])
    out["capture_path"] = {"what": "tests/test_capture_gpu.py: 24 train / 2 held-out views of a 26-frame capture through distorted per-frame cameras "
                                   "(PNG and JPEG), auto-scaled to about 1/4, near 0.5, far 1.5, uniform spacing",
                           "psnr_before": float(m.group(1)), "psnr_after": float(m.group(2)), "gain_db": float(m.group(3)),
                           "test_passed": res.returncode == 0}
    out["test_bound_db"] = round(0.5 * out["blender_path_on_parent"]["gain_db"], 4)
    return out


def main():
    from tests.test_capture_gpu import measure_against_float64

    worst, errors, checked = measure_against_float64()
    report = {"what": "the capture data path: rsn_sample_capture_rays / rsn_capture_rays_image (include/rsn.h, 'captures')",
              "device": torch.cuda.get_device_name(0),
              "accuracy": {"pixels": checked, "bound": "4 x the error of the float32 restatement of the recipe against float64, per camera and level",
                           "share_of_bound": {k: round(v, 4) for k, v in worst.items()}, "largest_errors": {k: float(f"{v:.4g}") for k, v in errors.items()}}}
    print(json.dumps(report["accuracy"]), flush=True)
    if ARGS.parent_tree is not None:
        report["timing"] = timings()
        if not ARGS.no_toy_scene:
            report["toy_scene"] = toy_scene()
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    if ARGS.child:
        child_blender_gain() if ARGS.arm == "blender_gain" else child_timing()
    else:
        main()
