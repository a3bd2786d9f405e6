"""Times and counts of one TSDF mesh export (profiles/tsdf_export.json).

    python tools/tsdf_export_report.py --out profiles/tsdf_export.json [--params tests/golden/params_trained_l8_w256.npz]
                                       [--resolution 256] [--size 800] [--views 8] [--radius 4] [--elevation 30]

Builds the model the parameter fixture belongs to, writes it as a trainer checkpoint into a temporary directory and measures, on an
orbit of `views` cameras of size x size pixels (the Blender scenes' field of view):
  - the depth pass (Model.get_surface_outputs_for_camera_ray_bundle) per view, beside the full eval pass
    (get_outputs_for_camera_ray_bundle) per frame in the same run, both at the same chunk size;
  - rsn_tsdf_integrate per launch, for one view and for all views in one call, and the bytes per second that implies from 16 bytes
    per grid vertex and launch plus the gathered depth (at most 4 bytes per vertex and view);
  - mesh.export_mesh(method="tsdf"): seconds per stage and the vertex and triangle counts before and after the filter.
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
from reflect_sampling_nerf_amd import mesh, render, trainer  # noqa: E402

BLENDER_FOV_X = 0.6911112070083618  # camera_angle_x of the Blender synthetic scenes


def _timed(fn, repeats):
    """-> milliseconds of each of `repeats` calls of fn, from events on the current stream."""
    out = []
    for _ in range(repeats):
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
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--elevation", type=float, default=30.0)
    ap.add_argument("--chunk", type=int, default=mesh.DEFAULT_RAY_CHUNK)
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--full-frames", type=int, default=2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("tsdf_export_report needs a GPU", file=sys.stderr)
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
    model.config.eval_num_rays_per_chunk = args.chunk
    S, V, res = args.size, args.views, args.resolution
    intr = render.pinhole(S, S, BLENDER_FOV_X)
    poses = render.orbit_path(V, (0.0, 0.0, 0.0), args.radius, args.elevation)
    cams = {"c2w": poses, "width": S, "height": S, "fx": intr[0], "fy": intr[1], "cx": intr[2], "cy": intr[3]}
    (nx, ny, nz), origin, spacing = mesh.grid_frame(mesh.DEFAULT_BOUNDS, res)
    trunc = mesh.DEFAULT_TRUNC_SPACINGS * float(spacing.max())
    near = float(model.config.collider_params["near_plane"])
    report = {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "resolution": [nx, ny, nz],
              "bounds": list(mesh.DEFAULT_BOUNDS), "views": V, "image": [S, S], "orbit": {"radius": args.radius, "elevation_deg": args.elevation},
              "mma": args.mma, "ray_chunk": args.chunk, "trunc": trunc, "min_weight": mesh.DEFAULT_MIN_WEIGHT, "near": near,
              "device": torch.cuda.get_device_name(0),
              "note": "milliseconds from device events after a warm-up; the full pass alternates its chunks over side streams "
                      "(get_outputs_for_camera_ray_bundle), the depth pass enqueues them on one stream"}
    poses_dev = torch.from_numpy(poses).to(dev)
    with torch.no_grad():
        warm = render.camera_rays(poses_dev[0], 64, 64, *render.pinhole(64, 64, BLENDER_FOV_X), dev)
        model.get_surface_outputs_for_camera_ray_bundle(warm, args.chunk)
        model.get_outputs_for_camera_ray_bundle(warm)
        torch.cuda.synchronize()
        depth = torch.empty(V, S * S, device=dev)

        def depth_view(i):
            rays = render.camera_rays(poses_dev[i], S, S, *intr, dev)
            depth[i] = model.get_surface_outputs_for_camera_ray_bundle(rays, args.chunk)["depth_fine"].reshape(-1)

        ms_depth = [_timed(lambda i=i: depth_view(i), 1)[0] for i in range(V)]
        ms_full = [_timed(lambda i=i: model.get_outputs_for_camera_ray_bundle(render.camera_rays(poses_dev[i % V], S, S, *intr, dev)), 1)[0]
                   for i in range(args.full_frames)]
        report["depth_pass_ms_per_view"] = {"median": float(np.median(ms_depth)), "all": ms_depth}
        report["full_pass_ms_per_frame"] = {"median": float(np.median(ms_full)), "all": ms_full}
        finite = torch.isfinite(depth)
        report["depth_fine"] = {"min": float(depth[finite].min()), "median": float(depth[finite].median()), "max": float(depth[finite].max())}
        # the fusion kernel alone, on the depth maps just rendered
        n_grid = nx * ny * nz
        tsdf = torch.zeros(nz, ny, nx, device=dev)
        weight = torch.zeros(nz, ny, nx, device=dev)
        launches = {}
        for n in sorted({1, V}):
            mesh.integrate_depth(tsdf, weight, origin, spacing, poses_dev[:n], depth[:n], S, S, *intr, trunc, near)  # warm-up
            ms = _timed(lambda n=n: mesh.integrate_depth(tsdf, weight, origin, spacing, poses_dev[:n], depth[:n], S, S, *intr, trunc, near), 5)
            med = float(np.median(ms))
            volume, gather = 16 * n_grid, 4 * n_grid * n
            launches[f"{n}_views"] = {"ms": ms, "median_ms": med, "volume_bytes": volume, "gather_bytes_at_most": gather,
                                      "bytes_per_second_volume": volume / (med * 1e-3),
                                      "bytes_per_second_volume_and_gather_at_most": (volume + gather) / (med * 1e-3)}
        report["integrate_launch"] = launches
        del tsdf, weight, depth
    with tempfile.TemporaryDirectory() as tmp:
        opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
        ckpt = trainer.save_checkpoint(trainer.checkpoint_path(tmp, 0), model, opt, 0)
        ply = os.path.join(tmp, "mesh.ply")
        small = dict(cams, width=32, height=32, **dict(zip(("fx", "fy", "cx", "cy"), render.pinhole(32, 32, BLENDER_FOV_X))))
        mesh.export_mesh(ckpt, ply, resolution=32, method="tsdf", cameras=small, mma=args.mma)  # warm-up
        r = mesh.export_mesh(ckpt, ply, resolution=res, method="tsdf", cameras=cams, mma=args.mma, ray_chunk=args.chunk, views_per_launch=V)
        sec = r["seconds"]
        report["export"] = {"seconds": sec, "integrate_launches": r["integrate_launches"], "depth_ms_per_view": 1e3 * sec["depth"] / V,
                            "integrate_ms_per_launch": 1e3 * sec["integrate"] / max(1, r["integrate_launches"]),
                            "extract_ms": 1e3 * (sec["count"] + sec["emit"]), "filter_ms": 1e3 * sec["filter"],
                            "vertices_extracted": r["vertices_extracted"], "triangles_extracted": r["triangles_extracted"],
                            "vertices": r["vertices"], "triangles": r["triangles"], "ply_bytes": os.path.getsize(ply)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
