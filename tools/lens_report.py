#!/usr/bin/env python3
"""What masks and fisheye cameras cost on the capture data path and how exact the fisheye rays are: profiles/capture_lens.json.

    python tools/lens_report.py --parent-tree DIR [--out profiles/capture_lens.json] [--images 100] [--blocks 3] [--steps 10]

Five measurements, all on the GPU (there is no fallback); none of them gates a test except the toy scene's gain:
  accuracy   tests/test_lens_gpu.measure_against_float64: every pixel of the tests' fisheye / perspective rows at levels 0 and 1, the
             kernel's error as a share of the tests' bound (4 x the error of the float32 restatement of the recipe + one fp32 ulp).
  lists      rsn_build_live_pixels (count, scan and fill) for --images images of 800 x 800 with 30 % of their 4 x 4 blocks live, at
             levels 1 and 4: 10 untimed calls, then 10 blocks of 10 calls between two HIP events.
  sampler    one training batch of 4096 rays from the same image set: rsn_sample_capture_rays of the parent commit's build (DIR: a
             built checkout of it) against rsn_sample_capture_rays_live of this one with all-live lists, with the 30 % mask and with a
             fisheye table, every perspective arm on the same distorted table.  Child processes that each import ONE tree, in the
             order parent / all_live / mask30 / fisheye / fisheye / mask30 / all_live / parent; per child 20 untimed calls, then 20
             blocks of 50 calls, each block between two HIP events.
  step       the headline training step (4096 rays x (128 + 128 + 64 + 64), 8 x 256, exact fp32; next_train + train_step, FusedRAdam
             with lr = 0) fed by each of the four, in the same children.
  toy_scene  the end-to-end test's own deterministic run (tests/test_lens_gpu.run_end_to_end): the held-out PSNR over live pixels
             before and after its training steps.  The test asks for half of this gain.  One run on a toy scene: a record, not a claim."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("parent", "all_live", "mask30", "fisheye")


def _args():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (without it: accuracy, lists and the toy scene)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "capture_lens.json"))
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-toy-scene", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--arm", default="all_live", choices=ARMS, help=argparse.SUPPRESS)
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
COEFFS = (-0.12, 0.03, -0.004, 0.002, -0.0015)  # the capture tests' k1 k2 k3 p1 p2
FISHEYE = (-0.03, 0.006, -0.001, 0.0002)  # the lens tests' k1 k2 k3 k4


def shell(n, radius=4.0):
    k = np.arange(n) + 0.5
    z = np.clip(0.8 * (1 - 2 * k / (n + 1)), -0.8, 0.8)
    phi = k * np.pi * (3 - np.sqrt(5))
    poses = []
    for p in radius * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1):
        back = p / np.linalg.norm(p)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        poses.append(np.concatenate([np.stack([right, np.cross(back, right), back], 1), p[:, None]], 1))
    return np.stack(poses).astype(np.float32)


def mask30(n):
    blocks = (np.random.default_rng(1).random((n, SIZE // 4, SIZE // 4)) < 0.3).astype(np.uint8)
    return np.kron(blocks, np.ones((4, 4), np.uint8))


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
    if ARGS.arm == "fisheye":  # an equidistant lens of the same focal length: theta_d = 0.51 at the corners
        scene.cameras = np.tile(np.float32([FOCAL, FOCAL, SIZE / 2, SIZE / 2, *FISHEYE[:3], 0, 0, FISHEYE[3], 1, 0]), (n, 1))
    else:
        scene.cameras = np.tile(np.float32([FOCAL, FOCAL, SIZE / 2, SIZE / 2, *COEFFS]), (n, 1))
    if ARGS.arm == "all_live":
        scene.masks = np.ones((n, SIZE, SIZE), np.uint8)
    elif ARGS.arm == "mask30":
        scene.masks = mask30(n)
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
    order = ["parent", "all_live", "mask30", "fisheye", "fisheye", "mask30", "all_live", "parent"]
    runs = []
    for arm in order:
        runs.append({"arm": arm, **run_child(arm, parent if arm == "parent" else HERE)})
        print(arm, statistics.median(runs[-1]["sampler_us_blocks"]), runs[-1]["ms_per_step_blocks"], flush=True)
    out = {"shape": {"rays": 4096, "images": ARGS.images, "size": [SIZE, SIZE], "samples": [128, 128, 64, 64], "layers": 8, "width": 256, "mma": "f32"},
           "arms": {"parent": f"the parent commit's build and package: rsn_sample_capture_rays, every row with (k1, k2, k3, p1, p2) = {COEFFS}",
                    "all_live": "rsn_sample_capture_rays_live, the same table, lists that hold every pixel",
                    "mask30": "rsn_sample_capture_rays_live, the same table, 30 % of the 4 x 4 blocks live",
                    "fisheye": f"rsn_sample_capture_rays_live, no lists, every row a fisheye one with (k1, k2, k3, k4) = {FISHEYE}"},
           "method": f"one process per run (a process binds one build), order {' / '.join(order)}; sampler: 20 untimed calls of next_train, then 20 "
                     f"blocks of 50 calls between two HIP events; step: {ARGS.warmup} untimed steps, then {ARGS.blocks} blocks of {ARGS.steps} steps "
                     "(next_train + train_step) between two HIP events, FusedRAdam with lr = 0",
           "runs": runs}
    for key, name, digits in (("sampler_us_blocks", "sampler_us", 3), ("ms_per_step_blocks", "ms_per_step", 4)):
        blocks = {a: [t for r in runs if r["arm"] == a for t in r[key]] for a in ARMS}
        med = {a: statistics.median(v) for a, v in blocks.items()}
        out[name] = {"median": {a: round(v, digits) for a, v in med.items()},
                     "spread": {a: round(max(v) - min(v), digits) for a, v in blocks.items()},
                     "per_run_median": {a: [round(statistics.median(r[key]), digits) for r in runs if r["arm"] == a] for a in ARMS},
                     "minus_parent": {a: round(med[a] - med["parent"], digits) for a in ARMS[1:]}}
    return out


def list_build():
    lib = _abi.load_library()
    n = ARGS.images
    masks = torch.from_numpy(mask30(n)).to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    out = {"shape": {"images": n, "size": [SIZE, SIZE], "live": "30 % of the 4 x 4 blocks"},
           "method": "count, scan and fill in one call; 10 untimed calls, then 10 blocks of 10 calls between two HIP events"}
    for levels in (1, 4):
        ws = torch.empty(lib.rsn_live_pixels_workspace_bytes(n, SIZE, SIZE, levels) // 4, device=DEV, dtype=torch.int32)
        counts = torch.zeros(levels, device=DEV, dtype=torch.int32)
        _abi.check(lib.rsn_build_live_pixels(n, SIZE, SIZE, levels, _abi.ptr(masks), None, 0, _abi.ptr(counts), _abi.ptr(ws), ws.numel() * 4, stream))
        host = counts.cpu().numpy().view(np.uint32).astype(np.int64)
        live = torch.empty(int(host.sum()), device=DEV, dtype=torch.int32)

        def build():
            _abi.check(lib.rsn_build_live_pixels(n, SIZE, SIZE, levels, _abi.ptr(masks), _abi.ptr(live), live.numel(), _abi.ptr(counts), _abi.ptr(ws),
                                                 ws.numel() * 4, stream))

        for _ in range(10):
            build()
        torch.cuda.synchronize()
        ms = [between_events(build, 10) for _ in range(10)]
        out[f"levels_{levels}"] = {"live_pixels": [int(c) for c in host], "ms_median": round(statistics.median(ms), 4),
                                   "ms_spread": round(max(ms) - min(ms), 4)}
    return out


def toy_scene():
    from tests.test_lens_gpu import E2E_FRAMES, run_end_to_end, write_masked_fisheye_sphere

    with tempfile.TemporaryDirectory() as tmp:
        root, _, rows, masks = write_masked_fisheye_sphere(os.path.join(tmp, "capture"))
        numbers, _ = run_end_to_end(root, rows, masks, tmp)
    return {"scene": f"Lambert sphere of radius 0.8 seen from a radius-4 shell through {E2E_FRAMES} fisheye cameras, written as the 48 x 48 images_2 of a "
                     "96 x 96 capture, the lower third of every view poisoned with magenta and masked out; 24 train / 2 held-out views; 4 x 64 "
                     "field, 32 + 32 + 16 + 16 samples, 1024 rays a step, deterministic mode",
            **{k: (v if isinstance(v, int) else round(float(v), 4)) for k, v in numbers.items()},
            "test_bound_db": round(0.5 * float(numbers["gain_db"]), 4), "note": "one run on a toy scene: a record, not a claim"}


def main():
    from tests.test_lens_gpu import measure_against_float64

    worst, errors, checked = measure_against_float64()
    report = {"what": "masks and fisheye cameras on the capture data path: rsn_build_live_pixels / rsn_sample_capture_rays_live / "
                      "rsn_capture_rays_image2 (include/rsn.h, 'captures: masks and fisheye lenses')",
              "device": torch.cuda.get_device_name(0),
              "accuracy": {"pixels": checked, "bound": "4 x the error of the float32 restatement of the recipe against float64 + one fp32 ulp, per row and level",
                           "share_of_bound": {k: round(v, 4) for k, v in worst.items()}, "largest_errors": {k: float(f"{v:.4g}") for k, v in errors.items()}}}
    print(json.dumps(report["accuracy"]), flush=True)
    report["lists"] = list_build()
    print(json.dumps(report["lists"]), flush=True)
    if not ARGS.no_toy_scene:
        report["toy_scene"] = toy_scene()
        print(json.dumps(report["toy_scene"]), flush=True)
    if ARGS.parent_tree is not None:
        report["timing"] = timings()
    os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
    with open(ARGS.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(f"wrote {ARGS.out}")


if __name__ == "__main__":
    if ARGS.child:
        child_timing()
    else:
        main()
