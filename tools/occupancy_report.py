"""What empty-space skipping saves on a rendered frame (profiles/occupancy_cull.json).

    python tools/occupancy_report.py --out profiles/occupancy_cull.json [--params tests/golden/params_trained_l8_w256.npz]
                                     [--size 800] [--frames 4] [--repeats 3] [--chunk 4096] [--resolution 128]

Builds the model the parameter fixture belongs to and renders a short orbit with render.render_path, seven channels, as the
`render` command does -- without and with an occupancy grid (occupancy.attach_occupancy: the box of the path's segments, the
defaults for sigma and dilation).  After one warm-up pass of each kind the two are timed alternately, `repeats` passes each:
wall time per frame of every pass (a host clock around work that ends in a device synchronise), and per culled frame the
milliseconds between the device events of the stages cull / gather / render (the chunks) / scatter.  Also recorded: the grid-build
time split into the field evaluation and the bit build (device events, after a warm-up build), the occupied share of cells, the
culled share of rays, and -- from one more pass of each kind that keeps the frames -- the PSNR and the largest difference between
the culled and the unculled final colour (8-bit panels, in units of 1/255 and as a fraction; per frame; and the share of pixels
that move by more than 2, 8 and 26 of 255, i.e. 0.008, 0.03 and 0.1).  The verdict compares the flagged
frame time with (1 - 0.5 * culled share) of the unflagged one.  Recorded values; the threshold is the issue's, not a tuned one.

    python tools/occupancy_report.py --samples --out profiles/occupancy_samples.json [--frames 2] [--repeats 2]
                                     [--chunks 4096 16384] [--mmas f32 bf16]

With --samples: per-sample skipping (model.occupancy_samples) on the same orbit, for every arithmetic of --mmas and chunk size of
--chunks, three modes timed alternately after a warm-up of each: plain, ray cull, ray cull plus sample skipping.  Recorded per
configuration: seconds per frame of every pass; for the third mode the milliseconds per frame between the device events around the
three stages of Field.evaluate_frustums_skipping (mark + compact, field, scatter), summed over its launches -- the chunks run on
side streams, so the sum can exceed the frame's wall time -- and per level; the live share of the sample slots per level; and,
for both culling modes against the plain render's 8-bit final colour, the PSNR, the share of pixels off by more than 0.03 and
the worst pixel.  "fixture_view" is the 40 x 40 view of tests/test_occupancy_samples_gpu.py in f32: the PSNR of the final colour
(float, clamped) with sample skipping against the plain render, which that test's floor is derived from."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import mesh, occupancy, render, trainer  # noqa: E402

STAGES = ("cull", "gather", "render", "scatter")
SAMPLE_STAGES = ("mark_compact", "field", "scatter")
MODES = ("plain", "ray_cull", "sample_skipping")


def _ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    r = fn()
    e.record()
    torch.cuda.synchronize()
    return r, s.elapsed_time(e)


def _quality(a, b, k, W):
    """8-bit panels a (plain) and b -> PSNR, share of pixels off by more than 0.03, worst pixel of the final colour (tile k)."""
    diffs = [np.abs(x[:, k * W:(k + 1) * W].astype(np.int32) - y[:, k * W:(k + 1) * W].astype(np.int32)) for x, y in zip(a, b)]
    mse = float(np.mean([np.mean((d / 255.0) ** 2) for d in diffs]))
    pixel = [d.max(axis=-1) for d in diffs]
    return {"psnr_db": float(10.0 * np.log10(1.0 / max(mse, 1e-12))),
            "share_of_pixels_over_0.03": float(np.mean([np.mean(p > 0.03 * 255.0) for p in pixel])),
            "worst_pixel": float(max(p.max() for p in pixel)) / 255.0}


def _fixture_view(state, layers, width):
    """The view of tests/test_occupancy_samples_gpu.py::test_quality_on_the_trained_fixture, measured the way it measures: the
    fixture's own sample counts (32 / 32 / 16 / 16), f32, the default chunk."""
    model = trainer.make_model(pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                                                  num_reflect_importance_samples=16, base_mlp_num_layers=layers,
                                                                  base_mlp_layer_width=width))
    model.field.load_state_dict(state, strict=True)
    model.to("cuda:0").eval()
    S = 40
    rays = render.camera_rays(render.orbit_path(1, (0.0, 0.0, 0.0), 4.0, 25.0, 30.0)[0], S, S, *render.pinhole(S, S, np.radians(50.0)), "cuda:0")
    rays.nears = torch.full((S, S, 1), 2.0, device="cuda:0")
    rays.fars = torch.full((S, S, 1), 6.0, device="cuda:0")
    model.occupancy, model.occupancy_samples = None, False
    plain = model.get_outputs_for_camera_ray_bundle(rays)["mid_reflect_fine"].clamp(0, 1)
    grid = model.occupancy = occupancy.build_occupancy(model.field, (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0), 96)
    out = {}
    for name, flag in (("ray_cull", False), ("sample_skipping", True)):
        model.occupancy_samples = flag
        diff = (model.get_outputs_for_camera_ray_bundle(rays)["mid_reflect_fine"].clamp(0, 1) - plain).reshape(S * S, 3)
        worst = diff.abs().amax(dim=1)
        out[name] = {"psnr_db": float(10.0 * torch.log10(1.0 / diff.double().pow(2).mean().clamp_min(1e-12))),
                     "share_of_pixels_over_0.03": float((worst > 0.03).float().mean()), "worst_pixel": float(worst.max())}
    live = grid.samples_live_dev.tolist()
    out["samples"] = {name: {"seen": grid.samples_seen[i], "live": live[i]} for i, name in enumerate(occupancy.LEVELS)}
    out["rays"], out["culled_share"], out["samples_per_level"] = S * S, grid.culled_share(), [32, 32, 16, 16]
    return out


def samples_report(args, model, state, layers, width) -> dict:
    H = W = args.size
    intr = render.pinhole(W, H, 0.6911112070083618)
    poses = render.orbit_path(args.frames, (0.0, 0.0, 0.0), args.radius, args.elevation)
    channels = render.DEFAULT_CHANNELS
    k = channels.index("rgb")
    settings = {"resolution": args.resolution, "sigma": occupancy.DEFAULT_SIGMA, "dilate": occupancy.DEFAULT_DILATE, "bounds": None}
    configs = []
    for mma in args.mmas:
        model.field.set_mma_mode(mma)
        grid = occupancy.attach_occupancy(model, settings, poses, H, W, *intr)  # from the field in this arithmetic
        for chunk in args.chunks:
            model.config.eval_num_rays_per_chunk = int(chunk)

            def one_pass(mode, keep=False):
                model.occupancy = None if mode == "plain" else grid
                model.occupancy_samples = mode == "sample_skipping"
                grid.sample_stage_events = [] if mode == "sample_skipping" else None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = render.render_path(model, poses, H, W, *intr, channels, None, None if keep else (lambda i, a: None))
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / args.frames
                events, grid.sample_stage_events = grid.sample_stage_events, None
                return wall, events, frames

            for mode in MODES:
                one_pass(mode)  # warm-up of every kind
            seconds = {m: [] for m in MODES}
            stage_ms = {s: [] for s in SAMPLE_STAGES}
            level_ms = {name: {s: [] for s in SAMPLE_STAGES} for name in occupancy.LEVELS}
            for _ in range(args.repeats):  # alternating: what else runs on the machine hits all three alike
                for mode in MODES:
                    wall, events, _ = one_pass(mode)
                    seconds[mode].append(wall)
                    if events:
                        for si, s_ in enumerate(SAMPLE_STAGES):
                            per_level = {name: 0.0 for name in occupancy.LEVELS}
                            for level_id, ev in events:
                                per_level[occupancy.LEVELS[level_id]] += ev[si].elapsed_time(ev[si + 1])
                            stage_ms[s_].append(sum(per_level.values()) / args.frames)
                            for name, v in per_level.items():
                                level_ms[name][s_].append(v / args.frames)
            seen0, live0 = list(grid.samples_seen), grid.samples_live_dev.tolist()
            kept = {mode: one_pass(mode, keep=True)[2] for mode in MODES}
            live1 = grid.samples_live_dev.tolist()
            share = {name: {"seen": grid.samples_seen[i] - seen0[i], "live": live1[i] - live0[i],
                            "live_share": (live1[i] - live0[i]) / max(grid.samples_seen[i] - seen0[i], 1)} for i, name in enumerate(occupancy.LEVELS)}
            med = {m: float(np.median(v)) for m, v in seconds.items()}
            configs.append({
                "mma": mma, "chunk": int(chunk), "seconds_per_frame": seconds, "median_seconds_per_frame": med,
                "ratio_sample_skipping_over_ray_cull": med["sample_skipping"] / med["ray_cull"],
                "ratio_sample_skipping_over_plain": med["sample_skipping"] / med["plain"],
                "sample_stage_ms_per_frame": {s_: float(np.mean(v)) for s_, v in stage_ms.items()},
                "sample_stage_ms_per_frame_by_level": {name: {s_: float(np.mean(v)) for s_, v in d.items()} for name, d in level_ms.items()},
                "samples": share,
                "final_colour_vs_plain": {m: _quality(kept["plain"], kept[m], k, W) for m in MODES[1:]},
                "grid": {kk: vv for kk, vv in grid.describe().items() if kk != "samples"},
            })
            print(json.dumps(configs[-1]), flush=True)
    model.field.set_mma_mode("f32")
    return {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "size": [W, H], "frames": args.frames,
            "repeats": args.repeats, "channels": list(channels), "orbit": {"radius": args.radius, "elevation_deg": args.elevation},
            "device": torch.cuda.get_device_name(0), "max_radius_rule": "max(dilate, 1) * min(spacing): a design rule, not measured",
            "configurations": configs, "fixture_view": _fixture_view(state, layers, width),
            "note": "seconds per frame: host clock around render_path of all frames, ending in a device synchronise, PNG encoding not "
                    "included; passes of the three kinds alternate; sample-stage times: device events around the three stages of every "
                    "evaluate_frustums_skipping, summed per frame over launches that overlap on side streams; `seen` counts every "
                    "sample slot of the launches, the rows behind a device-side count (culled and unreflected rays) included"}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", action="store_true", help="the three-mode study of per-sample skipping (see the module's docstring)")
    ap.add_argument("--chunks", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--mmas", nargs="+", default=["f32", "bf16"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--params", default=os.path.join(REPO, "tests", "golden", "params_trained_l8_w256.npz"))
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--resolution", type=int, default=occupancy.DEFAULT_RESOLUTION)
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--elevation", type=float, default=30.0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("occupancy_report needs a GPU", file=sys.stderr)
        return 2
    pz = np.load(args.params, allow_pickle=False)
    state = {k: torch.from_numpy(pz[k]) for k in pz.files}
    layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("mlp_base.layers."))
    width = int(state["mlp_base.layers.0.weight"].shape[0])
    model = trainer.make_model(pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=layers, base_mlp_layer_width=width))
    model.field.load_state_dict(state, strict=True)
    model.to("cuda:0").eval()
    if args.samples:
        report = samples_report(args, model, state, layers, width)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)
            fh.write("\n")
        return 0
    model.field.set_mma_mode(args.mma)
    model.config.eval_num_rays_per_chunk = int(args.chunk)
    H = W = args.size
    intr = render.pinhole(W, H, 0.6911112070083618)  # camera_angle_x of the Blender synthetic scenes
    poses = render.orbit_path(args.frames, (0.0, 0.0, 0.0), args.radius, args.elevation)
    channels = render.DEFAULT_CHANNELS
    settings = {"resolution": args.resolution, "sigma": occupancy.DEFAULT_SIGMA, "dilate": occupancy.DEFAULT_DILATE, "bounds": None}

    # the grid: a warm-up build, then the two parts timed apart
    grid = occupancy.attach_occupancy(model, settings, poses, H, W, *intr)
    bounds = grid.bounds
    torch.cuda.synchronize()
    vol, field_ms = _ms(lambda: mesh.density_grid(model.field, bounds, args.resolution))
    _, origin, spacing = mesh.grid_frame(bounds, args.resolution)
    grid, bits_ms = _ms(lambda: occupancy.occupancy_from_volume(vol, origin, spacing, settings["sigma"], settings["dilate"]))
    del vol

    def one_pass(with_grid, keep=False):
        model.occupancy = grid if with_grid else None
        events = model.occupancy_stage_events = [] if with_grid else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = render.render_path(model, poses, H, W, *intr, channels, None, None if keep else (lambda i, a: None))
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.frames
        model.occupancy_stage_events = None
        stages = [{s: ev[k].elapsed_time(ev[k + 1]) for k, s in enumerate(STAGES)} for ev in (events or [])]
        return wall, stages, frames

    one_pass(False)
    one_pass(True)  # warm-up of both kinds
    plain_s, culled_s, stage_rows = [], [], []
    for _ in range(args.repeats):  # alternating: what else runs on the machine hits both alike
        plain_s.append(one_pass(False)[0])
        wall, stages, _ = one_pass(True)
        culled_s.append(wall)
        stage_rows.extend(stages)
    seen0, hits0 = grid.rays_seen, int(grid.hits_dev.item())
    _, _, a = one_pass(False, keep=True)
    _, _, b = one_pass(True, keep=True)
    culled_share = 1.0 - (int(grid.hits_dev.item()) - hits0) / (grid.rays_seen - seen0)
    k = channels.index("rgb")
    diffs = [np.abs(x[:, k * W:(k + 1) * W].astype(np.int32) - y[:, k * W:(k + 1) * W].astype(np.int32)) for x, y in zip(a, b)]
    mse = float(np.mean([np.mean((d / 255.0) ** 2) for d in diffs]))
    worst = int(max(d.max() for d in diffs))
    pixel = [d.max(axis=-1) for d in diffs]  # per pixel, the largest of the three channels
    over = {f"share_of_pixels_over_{t}_255": float(np.mean([np.mean(p > t) for p in pixel])) for t in (2, 8, 26)}
    near, far = occupancy.eval_planes(model)
    plain, culled = float(np.median(plain_s)), float(np.median(culled_s))
    bound = 1.0 - 0.5 * culled_share
    report = {
        "params": os.path.relpath(args.params, REPO), "network": [layers, width], "mma": args.mma, "size": [W, H], "frames": args.frames,
        "repeats": args.repeats, "chunk": args.chunk, "channels": list(channels), "orbit": {"radius": args.radius, "elevation_deg": args.elevation},
        "device": torch.cuda.get_device_name(0),
        "grid": {**grid.describe(), "culled_share": culled_share, "build_ms": {"field_evaluation": field_ms, "bit_build": bits_ms}},
        "seconds_per_frame": {"without": plain_s, "with_skip_empty": culled_s, "median_without": plain, "median_with": culled,
                              "spread_without": max(plain_s) - min(plain_s), "spread_with": max(culled_s) - min(culled_s)},
        "stage_ms_per_frame": {"mean": {s: float(np.mean([r[s] for r in stage_rows])) for s in STAGES},
                               "min": {s: float(np.min([r[s] for r in stage_rows])) for s in STAGES},
                               "max": {s: float(np.max([r[s] for r in stage_rows])) for s in STAGES}},
        "segments": {"near": near, "far": far},
        "final_colour_culled_vs_unculled": {"psnr_db": float(10.0 * np.log10(1.0 / max(mse, 1e-12))), "largest_difference_255": worst,
                                            "largest_difference": worst / 255.0,
                                            "largest_difference_255_per_frame": [int(d.max()) for d in diffs], **over},
        "ratio_with_over_without": culled / plain, "accepted_at_most": bound, "accepted": bool(culled / plain <= bound),
        "note": "seconds per frame: host clock around render_path of all frames, ending in a device synchronise, PNG encoding not "
                "included; passes of the two kinds alternate; stage times between device events of the culled frames",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
