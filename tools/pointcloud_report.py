"""Times and counts of one point-cloud export (profiles/pointcloud_export.json).

    python tools/pointcloud_report.py --out profiles/pointcloud_export.json [--params tests/golden/params_trained_l8_w256.npz]
                                      [--resolution 512] [--size 800] [--views 8] [--radius 4] [--elevation 30]

Builds the model the parameter fixture belongs to, writes it as a trainer checkpoint into a temporary directory and measures, on an
orbit of `views` cameras of size x size pixels (the Blender scenes' field of view) and a grid of resolution^3 cells on the default box:
  - the depth pass (Model.get_surface_outputs_for_camera_ray_bundle) per view;
  - rsn_pointcloud_mark and rsn_pointcloud_select for all views in one call each, on the maps just rendered, and the bytes per second
    their MINIMUM traffic implies: mark reads depth and accumulation (8 bytes per pixel) and touches 4 bytes of owner per candidate;
    select reads the same 8 bytes per pixel and 4 per candidate, writes and reads one flag byte per pixel and writes 16 bytes per
    kept point.  The re-read neighbour depths, the poses and the tile counts are not counted;
  - pointcloud.export_pointcloud: seconds per stage, candidates and points.
The launch of rsn_tsdf_integrate for the same eight views (profiles/tsdf_export.json) is copied beside them when that file is there.
Times are from device events after a warm-up.  Recorded values; no threshold and no ratio is asserted."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import mesh, pointcloud, render, trainer  # noqa: E402

BLENDER_FOV_X = 0.6911112070083618  # camera_angle_x of the Blender synthetic scenes


def _timed(fn, repeats, before=None):
    """-> milliseconds of each of `repeats` calls of fn, from events on the current stream; `before` runs untimed ahead of each."""
    out = []
    for _ in range(repeats):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--params", default=os.path.join(REPO, "tests", "golden", "params_trained_l8_w256.npz"))
    ap.add_argument("--resolution", type=int, default=pointcloud.DEFAULT_RESOLUTION)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--chunk", type=int, default=mesh.DEFAULT_RAY_CHUNK)
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("pointcloud_report needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda:0")
    pz = np.load(args.params, allow_pickle=False)
    state = {k: torch.from_numpy(pz[k]) for k in pz.files}
    layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("mlp_base.layers."))
    width = int(state["mlp_base.layers.0.weight"].shape[0])
    model = trainer.make_model(pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=layers, base_mlp_layer_width=width))
    model.field.load_state_dict(state, strict=True)
    model.to(dev).eval()
    model.field.set_mma_mode(args.mma)
    S, V = args.size, args.views
    intr = render.pinhole(S, S, BLENDER_FOV_X)
    poses = render.orbit_path(V, (0.0, 0.0, 0.0), args.radius, args.elevation)
    cams = {"c2w": poses, "width": S, "height": S, "fx": intr[0], "fy": intr[1], "cx": intr[2], "cy": intr[3]}
    dims, origin, spacing = pointcloud.cell_frame(mesh.DEFAULT_BOUNDS, args.resolution)
    min_acc, edge = pointcloud.DEFAULT_MIN_ACCUMULATION, pointcloud.DEFAULT_EDGE
    report = {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "resolution": list(dims),
              "bounds": list(mesh.DEFAULT_BOUNDS), "views": V, "image": [S, S], "orbit": {"radius": args.radius, "elevation_deg": args.elevation},
              "mma": args.mma, "ray_chunk": args.chunk, "min_accumulation": min_acc, "edge": edge, "device": torch.cuda.get_device_name(0),
              "note": "milliseconds from device events after a warm-up; bytes per second from the minimum traffic named in the tool's text"}
    poses_dev = torch.from_numpy(poses).to(dev)
    with torch.no_grad():
        warm = render.camera_rays(poses_dev[0], 64, 64, *render.pinhole(64, 64, BLENDER_FOV_X), dev)
        model.get_surface_outputs_for_camera_ray_bundle(warm, args.chunk)
        torch.cuda.synchronize()
        depth, acc = torch.empty(V, S * S, device=dev), torch.empty(V, S * S, device=dev)

        def depth_view(i):
            surf = model.get_surface_outputs_for_camera_ray_bundle(render.camera_rays(poses_dev[i], S, S, *intr, dev), args.chunk)
            depth[i], acc[i] = surf["depth_fine"].reshape(-1), surf["accumulation_fine"].reshape(-1)

        ms_depth = [_timed(lambda i=i: depth_view(i), 1)[0] for i in range(V)]
        report["depth_pass_ms_per_view"] = {"median": float(np.median(ms_depth)), "all": ms_depth}
        report["accumulation_fine"] = {"min": float(acc.min()), "median": float(acc.median()), "max": float(acc.max()),
                                       "share_at_least_min_accumulation": float((acc >= min_acc).float().mean())}
        # the two calls alone, all views in one call each, on the maps just rendered
        views = (dims, origin, spacing, poses_dev, depth, acc, S, S, *intr, 0, min_acc, edge)
        owner = pointcloud.new_owner(dims, dev)
        pixels = V * S * S
        rows = (torch.empty(2, device=dev, dtype=torch.int32), torch.empty(pixels, device=dev, dtype=torch.int32),
                torch.empty(pixels, 3, device=dev), torch.empty(int(pkg.load_library().rsn_pointcloud_workspace_bytes(V, S, S)),
                                                                 device=dev, dtype=torch.uint8))
        ms_mark = _timed(lambda: pointcloud.mark(owner, *views), args.repeats + 1, before=lambda: owner.fill_(pointcloud.NO_OWNER))[1:]
        candidates = int(pointcloud.select(None, *views, out=rows)[0][1].item())
        ms_all = _timed(lambda: pointcloud.select(None, *views, out=rows), args.repeats + 1)[1:]
        ms_thin = _timed(lambda: pointcloud.select(owner, *views, out=rows), args.repeats + 1)[1:]
        kept = int(rows[0][0].item())
        calls = {}
        for name, ms, traffic in (("mark", ms_mark, 8 * pixels + 4 * candidates),
                                  ("select_without_owner", ms_all, 10 * pixels + 16 * candidates),
                                  ("select", ms_thin, 10 * pixels + 4 * candidates + 16 * kept)):
            med = float(np.median(ms))
            calls[name] = {"ms": ms, "median_ms": med, "minimum_traffic_bytes": traffic, "bytes_per_second": traffic / (med * 1e-3)}
        report["calls"] = {"pixels": pixels, "candidates": candidates, "points": kept, "owner_bytes": 4 * owner.numel(), **calls}
        del owner, rows, depth, acc
    tsdf = os.path.join(REPO, "profiles", "tsdf_export.json")
    if os.path.isfile(tsdf):
        with open(tsdf) as fh:
            launch = json.load(fh).get("integrate_launch", {}).get(f"{V}_views")
        if launch:
            report["tsdf_integrate_launch_ms_for_comparison"] = {"median_ms": launch["median_ms"], "from": "profiles/tsdf_export.json",
                                                                 "note": "256^3 vertices, the same views: 16 bytes per vertex"}
    with tempfile.TemporaryDirectory() as tmp:
        opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
        ckpt = trainer.save_checkpoint(trainer.checkpoint_path(tmp, 0), model, opt, 0)
        ply = os.path.join(tmp, "cloud.ply")
        small = dict(cams, width=32, height=32, **dict(zip(("fx", "fy", "cx", "cy"), render.pinhole(32, 32, BLENDER_FOV_X))))
        pointcloud.export_pointcloud(ckpt, ply, small, resolution=32, mma=args.mma)  # warm-up
        r = pointcloud.export_pointcloud(ckpt, ply, cams, resolution=args.resolution, mma=args.mma, ray_chunk=args.chunk, views_per_launch=V)
        report["export"] = {"seconds": r["seconds"], "candidates": r["candidates"], "points": r["points"], "thin": r["thin"],
                            "depth_ms_per_view": 1e3 * r["seconds"]["depth"] / V, "ply_bytes": os.path.getsize(ply)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
