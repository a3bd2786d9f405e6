#!/usr/bin/env python3
"""Cost of the standalone data path (GPU box).

Leg A: the training step (default sample counts, 8 x 256) fed by RayDataManager.next_train -- one rsn_sample_camera_rays launch
per step -- against the same step on a pre-staged ray batch (drawn once by the same sampler, reused every step), the two
alternated in one process over several rounds and timed with HIP events, at each --rays and --mma.
Leg B (--profile): a child process under `rocprofv3 --kernel-trace --stats` that launches rsn_sample_camera_rays (4096 rays)
and rsn_ssim (800 x 800) --kernel-reps times each; the per-kernel averages are read from its stats CSV.

Usage: python tools/data_path_bench.py [--rays 1024,4096] [--mma f32,bf16] [--steps 20] [--warmup 5] [--rounds 6]
                                       [--profile] [--json out.json]
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402


def bench_scene(n_images=100, size=800, seed=0):
    """NeRF-synthetic-sized stand-in: 100 RGBA 800 x 800 images of noise on a radius-4 shell (timing only)."""
    from reflect_sampling_nerf_amd.data import BlenderScene

    rng = np.random.default_rng(seed)
    ims = rng.integers(0, 256, size=(n_images, size, size, 4), dtype=np.uint8)
    poses = np.zeros((n_images, 3, 4), np.float32)
    for i in range(n_images):
        back = rng.normal(size=3)
        back /= np.linalg.norm(back)
        right = np.cross([0.0, 0.0, 1.0], back)
        right /= np.linalg.norm(right)
        poses[i] = np.concatenate([np.stack([right, np.cross(back, right), back], 1), 4.0 * back[:, None]], 1)
    focal = 0.5 * size / math.tan(0.5 * 0.6911112070083618)
    return BlenderScene.from_arrays(ims, poses, focal=focal)


def step_legs(scene, R, mma, steps, warmup, rounds):
    import reflect_sampling_nerf_amd as pkg
    from reflect_sampling_nerf_amd.data import RayDataManager
    from reflect_sampling_nerf_amd.parallel import train_step

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = pkg.ReflectSamplingNeRFModelConfig().setup(scene_box=None, num_train_data=1).to(dev).train()
    model.field.set_mma_mode(mma)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)
    dm = RayDataManager(scene, dev, num_rays_per_batch=R, seed=0)
    staged_rb, staged_batch = dm.next_train(10**6)
    state = {"it": 100}

    def run(leg, n):
        for _ in range(n):
            if leg == "data":
                rb, batch = dm.next_train(state["it"])
            else:
                rb, batch = pkg.RayBundle(origins=staged_rb.origins, directions=staged_rb.directions,
                                          pixel_area=staged_rb.pixel_area), staged_batch
            train_step(model, rb, batch, opt, None, state["it"])
            state["it"] += 1

    times = {"data": [], "staged": []}
    for leg in ("data", "staged"):
        run(leg, warmup)
    torch.cuda.synchronize()
    for r in range(rounds):
        for leg in (("data", "staged") if r % 2 == 0 else ("staged", "data")):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(leg, steps)
            b.record()
            b.synchronize()
            times[leg].append(a.elapsed_time(b) / steps)
    out = {"rays": R, "mma": mma, "steps_per_round": steps, "rounds": rounds}
    for leg, v in times.items():
        out[leg + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "rounds": v}
    out["data_minus_staged_ms"] = out["data_ms"]["median"] - out["staged_ms"]["median"]
    del model, opt, dm
    torch.cuda.empty_cache()
    return out


def kernel_reps(reps):
    """The workload of the profiled child: the sampler at 4096 rays and SSIM at 800 x 800, `reps` launches each."""
    from reflect_sampling_nerf_amd import metrics
    from reflect_sampling_nerf_amd.data import RayDataManager

    dev = torch.device("cuda:0")
    dm = RayDataManager(bench_scene(), dev, num_rays_per_batch=4096)
    g = torch.Generator(dev).manual_seed(0)
    a = torch.rand(800, 800, 3, device=dev, generator=g)
    b = (a + 0.1 * torch.rand(800, 800, 3, device=dev, generator=g)).clamp(0, 1)
    for i in range(reps):
        dm.next_train(i)
        metrics.ssim(a, b)
    torch.cuda.synchronize()


def profile(reps, out_dir):
    """rocprofv3 run of kernel_reps() in a child process; its stats CSV is kept under out_dir/rocprof."""
    d = os.path.join(out_dir, "rocprof")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
           os.path.abspath(__file__), "--kernels-child", str(reps)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if res.returncode != 0:
        raise RuntimeError(f"rocprofv3 exited {res.returncode}:\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}")
    paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise RuntimeError(f"rocprofv3 wrote no kernel_stats.csv under {d}:\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    with open(max(paths, key=os.path.getmtime)) as fh:
        rows = list(csv.DictReader(fh))
    out = {}
    for row in rows:
        name = row["Name"]
        for key in ("rsn_sample_camera_rays_kernel", "rsn_ssim_tile_kernel", "rsn_ssim_reduce_kernel"):
            if key in name:
                out[key] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                            "min_us": float(row["MinNs"]) / 1e3, "max_us": float(row["MaxNs"]) / 1e3}
    if "rsn_ssim_tile_kernel" in out and "rsn_ssim_reduce_kernel" in out:
        out["ssim_800x800_total_avg_us"] = out["rsn_ssim_tile_kernel"]["avg_us"] + out["rsn_ssim_reduce_kernel"]["avg_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", default="1024,4096")
    ap.add_argument("--mma", default="f32,bf16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--profile", action="store_true", help="also run the rocprofv3 kernel-time leg")
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--kernels-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.kernels_child:
        kernel_reps(args.kernels_child)
        return
    assert torch.cuda.is_available(), "data_path_bench needs the GPU"
    scene = bench_scene()
    res = {"device": torch.cuda.get_device_name(0), "scene": "100 x 800 x 800 RGBA", "model": "8 x 256, samples 128/128/64/64",
           "step": []}
    for mma in args.mma.split(","):
        for R in (int(r) for r in args.rays.split(",")):
            row = step_legs(scene, R, mma, args.steps, args.warmup, args.rounds)
            print(json.dumps({k: row[k] for k in ("rays", "mma", "data_minus_staged_ms")}) +
                  f"  data {row['data_ms']['rounds']}  staged {row['staged_ms']['rounds']}", flush=True)
            res["step"].append(row)
    if args.profile:
        out_dir = os.path.dirname(os.path.abspath(args.json)) if args.json else tempfile.mkdtemp()
        res["kernels"] = profile(args.kernel_reps, out_dir)
        print(json.dumps(res["kernels"]), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
