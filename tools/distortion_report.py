#!/usr/bin/env python3
"""What the opt-in distortion loss costs and does (trainer --distortion-loss; rsn_distortion_forward / _backward): profiles/distortion.json.

    python tools/distortion_report.py --parent-tree DIR [--out profiles/distortion.json] [--images 24] [--blocks 4] [--steps 10]

Three measurements, all on the GPU (there is no fallback):
  kernels   rsn_distortion_forward and rsn_distortion_backward (accumulate = 1) at the headline shape, 4096 rays x 128 samples, on the
            weights rsn_composite makes of seeded densities: each call between two HIP events after 3 untimed calls, median of 20.
  step      the headline training step (4096 rays x (128 + 128 + 64 + 64), 8 x 256, exact fp32; next_train + train_step) in child
            processes that each import ONE tree: the parent commit's (DIR: a built checkout of it, which has no such term) and this
            one with the term off, on the fine level, and on both levels, in the order parent / off / fine / both / both / fine / off /
            parent.  A child runs --warmup untimed steps, then --blocks blocks of --steps steps, each block between two HIP events.  A
            process binds one build of the library, so the arms alternate per process and not per block.  The optimiser runs with
            lr = 0: the term changes what the model learns and with it the number of reflected rays, which is work of the step that
            these kernels do not do; with the parameters held every arm has the same work.
  toy_scene the Lambert sphere of the tests (24 train / 4 test views of 48 x 48), 400 deterministic steps with --distortion-loss 0.01
            and without: the mean L_ray of the test views' fine level (training-mode forward of every test view's rays, fixed jitter
            seed) and the test PSNR, beside the untrained model.  One run each: a record, not a claim."""
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
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "distortion.json"))
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
COEF = 0.01                  # mip-NeRF 360's coefficient; not measured on this method


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
    fine, coarse = ARMS[ARGS.arm]
    for key, coef in (("distortion_loss_fine", fine), ("distortion_loss_coarse", coarse)):
        if coef is not None:
            model.config.loss_coefficients[key] = coef
    # lr = 0: the optimiser launch runs and changes nothing.  The term changes what the model learns, with it the number of reflected
    # rays and so the step's work (measured with lr = 1e-3: +6.4 ms after 120 steps on noise images, none of it in these kernels);
    # with the parameters held every arm does the same work
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=0.0, eps=1e-15)
    dm = RayDataManager(blender_like_scene(ARGS.images), DEV, num_rays_per_batch=4096, seed=0)
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
def kernel_times():
    R, S = 4096, 128
    g = torch.Generator().manual_seed(0)
    sigma = (torch.rand(R, S, generator=g) * 8.0 * (torch.rand(R, S, generator=g) > 0.5)).to(DEV)
    nears, fars = torch.full((R,), 2.0, device=DEV), torch.full((R,), 6.0, device=DEV)
    sb, eb = ops.sample_spaced(R, None, S, 0, 1.0, nears, fars, torch.rand(R, S + 1, generator=g).to(DEV))
    w = ops.composite(R, None, S, 0, 0, sigma, eb, torch.zeros(R, S, 3, device=DEV), want_depth=False)["weights"]
    g_ray = torch.full((R,), COEF / R, device=DEV)
    g_sigma = torch.zeros(R, S, device=DEV)
    calls = {"rsn_distortion_forward": lambda: ops.distortion_forward(R, None, S, sb, w),
             "rsn_distortion_backward": lambda: ops.distortion_backward(R, None, S, sb, eb, sigma, g_ray, g_sigma, accumulate=True)}
    out = {"shape": {"rays": R, "samples": S}, "method": "one call between two HIP events, median of 20 after 3 untimed"}
    for name, call in calls.items():
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        t = sorted(between_events(call) * 1e3 for _ in range(20))
        out[name] = {"median_us": round(statistics.median(t), 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2)}
    return out


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
            "ms_per_step_by_block": {a: [round(statistics.mean(r["ms_per_step_blocks"][i] for r in runs if r["arm"] == a), 4)
                                         for i in range(ARGS.blocks)] for a in ARMS},  # the blocks of a run drift alike in every arm
            "minus_parent_ms": {a: round(med[a] - med["parent"], 4) for a in ("off", "fine", "both")},
            "minus_off_ms": {a: round(med[a] - med["off"], 4) for a in ("fine", "both")}}


def toy_scene(tmp):
    from reflect_sampling_nerf_amd import trainer
    from tests.test_pyramid_gpu import _cfg, _sphere_scene, _untrained_checkpoint

    steps = 400
    train_scene, test_scene = _sphere_scene(24), _sphere_scene(4, offset=0.37)
    kw = dict(steps=steps, rays=1024, save_every=0, log_every=0, seed=0, device=DEV, log=None, deterministic=True)
    cks = {"untrained": _untrained_checkpoint(os.path.join(tmp, "init")),
           "distortion_loss_0.01": trainer.train(train_scene, os.path.join(tmp, "on"), model_config=_cfg(), distortion_loss=COEF, **kw),
           "without": trainer.train(train_scene, os.path.join(tmp, "off"), model_config=_cfg(), **kw)}
    out = {"scene": "Lambert sphere, 24 train / 4 test views of 48 x 48; 4 x 64 field, 32 + 32 + 16 + 16 samples", "steps": steps, "rays": 1024,
           "deterministic": True, "coefficient": COEF,
           "mean_l_ray_fine": "mean over the rays of the 4 test views of the fine level's L_ray (rsn_distortion_forward in a training-mode "
                              "forward, jitter seed 0)",
           "note": "one run each on a toy scene: a record, not a claim"}
    dm = RayDataManager(test_scene, DEV)
    n_pix = test_scene.height * test_scene.width
    for name, ck in cks.items():
        r = trainer.evaluate(test_scene, ck, device=DEV, model_config=_cfg())["results"]
        model, _ = trainer.load_checkpoint(ck, _cfg(), DEV)
        model.train()
        model.config.loss_coefficients["distortion_loss_fine"] = COEF  # switches the fine level's forward launch on
        torch.manual_seed(0)
        per_view = []
        with torch.no_grad():
            for i in range(test_scene.num_images):
                rays = dm.camera_ray_bundle(i, 0).get_row_major_sliced_ray_bundle(0, n_pix)
                per_view.append(float(model(rays).fused["dist_loss_ray_fine"].double().mean()))
        out[name] = {"psnr": round(r["psnr"], 4), "coarse_psnr": round(r["coarse_psnr"], 4), "fine_ssim": round(r["fine_ssim"], 4),
                     "mean_l_ray_fine": float(f"{statistics.mean(per_view):.6g}")}
    return out


def main():
    import tempfile

    assert torch.cuda.is_available(), "tools/distortion_report.py needs a GPU"
    pkg.load_library()
    report = {"tool": "tools/distortion_report.py", "device": torch.cuda.get_device_name(0)}
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
