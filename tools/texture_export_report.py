"""Times, sizes and counts of textured mesh exports (profiles/texture_export.json).

    python tools/texture_export_report.py --out profiles/texture_export.json [--params tests/golden/params_trained_l8_w256.npz]
                                          [--resolutions 256 64] [--texels 8] [--iso 10] [--quantile 0.9] [--repeats 20]

Builds the model the parameter fixture belongs to, writes it as a trainer checkpoint into a temporary directory and, per resolution,
runs mesh.export_mesh(texture=True) on the density route -- at --iso, or, where the density never reaches it (the fixture's largest
density is below the default level), at the --quantile of the grid's densities, the level profiles/mesh_export.json uses -- and
records
  - the seconds per stage: atlas, bake and write beside grid, count, emit and attributes of the same run;
  - rsn_texture_points alone on the run's mesh: device events around each of `repeats` launches after a warm-up, the median, and the
    bytes per second that implies from its minimum traffic -- the reads of triangles (12 bytes each) and positions (12 bytes per
    vertex) once, and the 20 bytes every texel writes; beside it, in the same process, torch's device-to-device copy of the point buffer
    (bytes read plus written per second) as the yardstick, and the time of the list of live texels that texture_atlas builds after
    the launch.  Repeated launches write the same buffers: a texture under 256 MB stays in the last-level cache, and its rate is
    not a memory rate;
  - the texture's size, the share of live texels, the sizes of the six files and the PNG encoding time of the four maps (their pixels encoded
    again into memory, on the host: the part of `write` that is not the OBJ text).
Recorded values; no threshold and no ratio is asserted."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import mesh, texture, trainer  # noqa: E402


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
    from PIL import Image

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--params", default=os.path.join(REPO, "tests", "golden", "params_trained_l8_w256.npz"))
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--texels", type=int, default=texture.DEFAULT_TEXELS)
    ap.add_argument("--iso", type=float, default=mesh.DEFAULT_ISO)
    ap.add_argument("--quantile", type=float, default=0.9, help="the level where --iso lies above every density of the grid")
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("texture_export_report needs a GPU", file=sys.stderr)
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
    report = {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "bounds": list(mesh.DEFAULT_BOUNDS),
              "iso": args.iso, "quantile": args.quantile, "texels": args.texels, "mma": args.mma, "device": torch.cuda.get_device_name(0),
              "note": "seconds per stage from device events (write: host clock); rsn_texture_points: milliseconds from device events "
                      "around single launches after a warm-up; --texels 8 and the default --min-footprint are starting points that "
                      "have not been measured on a real scene, and this fixture is not one",
              "runs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
        ckpt = trainer.save_checkpoint(trainer.checkpoint_path(tmp, 0), model, opt, 0)

        def level_for(res):
            with torch.cuda.device(dev):
                vol = mesh.density_grid(model.field, mesh.DEFAULT_BOUNDS, res).reshape(-1)
                if bool((vol >= args.iso).any()):
                    return args.iso, "iso"
                return float(torch.quantile(vol[:: max(1, vol.numel() // (1 << 22))].double(), args.quantile)), f"p{100 * args.quantile:g}"

        mesh.export_mesh(ckpt, os.path.join(tmp, "warm.obj"), resolution=24, iso=level_for(24)[0], mma=args.mma, texture=True,
                         texels=args.texels)  # warm-up
        for res in args.resolutions:
            out = os.path.join(tmp, f"mesh{res}.obj")
            iso, level = level_for(res)
            print(f"resolution {res}: level {iso:g} ({level}); exporting", flush=True)
            r = mesh.export_mesh(ckpt, out, resolution=res, iso=iso, mma=args.mma, texture=True, texels=args.texels)
            print(f"resolution {res}: {r['triangles']} triangles, {r['texture_size']}^2 texels, seconds {r['seconds']}", flush=True)
            N = r["texture_size"]
            run = {"resolution": r["resolution"], "level": iso, "level_from": level, "vertices": r["vertices"], "triangles": r["triangles"], "seconds": r["seconds"],
                   "texture_size": N, "squares_per_row": N // args.texels, "live_texels": r["live_texels"],
                   "live_share": r["live_texels"] / float(N * N), "min_footprint": r["min_footprint"],
                   "file_bytes": {k: os.path.getsize(p) for k, p in r["files"].items()}}
            pixels = [np.asarray(Image.open(r["files"][name])) for name in texture.MAPS]
            t0 = time.time()
            for px in pixels:
                Image.fromarray(px).save(io.BytesIO(), format="PNG")
            run["png_encode_seconds_four_maps"] = time.time() - t0
            del pixels
            # the kernel alone, on the mesh of this run
            (nx, ny, nz), origin, spacing = mesh.grid_frame(mesh.DEFAULT_BOUNDS, res)
            with torch.cuda.device(dev):
                surface = mesh.extract_surface(mesh.density_grid(model.field, mesh.DEFAULT_BOUNDS, res), iso, origin, spacing)
                pos, tri = surface["positions"], surface["triangles"]
                texture.texture_atlas(pos, tri, args.texels)  # warm-up (and the buffers' first touch)
                ms = _timed(lambda: texture.texture_atlas(pos, tri, args.texels), 3)  # with its allocations and the live list
                lib, Q = pkg.load_library(), N // args.texels
                face = torch.empty(N * N, device=dev, dtype=torch.int32)
                point = torch.empty(N * N * 3, device=dev)
                fp = torch.empty(N * N, device=dev)
                stream = torch.cuda.current_stream().cuda_stream

                def launch():
                    rc = lib.rsn_texture_points(pos.shape[0], pos.data_ptr(), tri.shape[0], tri.data_ptr(), args.texels, Q,
                                                face.data_ptr(), point.data_ptr(), fp.data_ptr(), stream)
                    assert rc == 0, lib.rsn_last_error()

                if tri.shape[0]:
                    for _ in range(3):
                        launch()
                    torch.cuda.synchronize()
                    k_ms = _timed(launch, args.repeats)
                    traffic = 12 * int(tri.shape[0]) + 12 * int(pos.shape[0]) + 20 * N * N
                    med = float(np.median(k_ms))
                    # a yardstick measured here, in the same process: torch's device-to-device copy of the point buffer
                    other = torch.empty_like(point)
                    other.copy_(point)
                    c_ms = float(np.median(_timed(lambda: other.copy_(point), args.repeats)))
                    copy_rate = 2 * point.numel() * 4 / (c_ms * 1e-3)
                    del other
                    live_ms = _timed(lambda: torch.nonzero(face >= 0), 3)  # what texture_atlas does after the launch; ends in a host read
                    run["rsn_texture_points"] = {"ms": k_ms, "median_ms": med, "min_ms": float(min(k_ms)), "minimum_traffic_bytes": traffic,
                                                 "bytes_per_second": traffic / (med * 1e-3),
                                                 "device_copy": {"bytes_read_and_written": 2 * point.numel() * 4, "median_ms": c_ms,
                                                                 "bytes_per_second": copy_rate},
                                                 "share_of_device_copy_rate": traffic / (med * 1e-3) / copy_rate,
                                                 "buffers_fit_last_level_cache_256MB": bool(20 * N * N < 256 * 2 ** 20)}
                    run["live_list_ms"] = live_ms
                run["texture_atlas_call_ms"] = ms
                del face, point, fp, surface
            report["runs"][str(res)] = run
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
