"""Times and counts of the mesh decimation and of textured exports with and without it (profiles/mesh_decimate.json).

    python tools/decimate_report.py --out profiles/mesh_decimate.json [--params tests/golden/params_trained_l8_w256.npz]
                                    [--resolution 256] [--target-faces 50000] [--decimate-cells 64] [--repeats 7] [--exports 2]

Builds the model the parameter fixture belongs to, writes it as a trainer checkpoint into a temporary directory, extracts the density
route's mesh at --resolution -- at --iso, or, where the density never reaches it (the fixture's largest density is below the default
level), at the --quantile of the grid's densities, the level profiles/mesh_export.json and profiles/texture_export.json use -- and
records
  - decimate.decimate_to at --target-faces and decimate.decimate at --decimate-cells on that mesh: the milliseconds of every stage
    (search: all probes; cluster, sort, resolve, count, emit: the final pass) from device events at the stage boundaries, `repeats`
    runs after a warm-up, every run and the median; the host's clock around each whole call, ending in a synchronise; the probes
    made, and the counts before and after;
  - the whole textured export (mesh.export_mesh(texture=True)) without and with --target-faces, `exports` of each, run alternately
    in this one process: the seconds per stage, the atlas size, the live texels and the bytes of the files.
Recorded values; no threshold and no ratio is asserted.  The fixture is not a real scene: nothing here says what the reduction does
to rendered appearance, whether the cluster-cell footprint is the right one, or how the meshes compare with an edge-collapse
simplifier's."""
import argparse
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
from reflect_sampling_nerf_amd import decimate, mesh, texture, trainer  # noqa: E402


class _Marks:
    """Device events at the stage boundaries of one call."""

    def __init__(self):
        self.names, self.events = [], [self._event()]

    @staticmethod
    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def __call__(self, name):
        self.names.append(name)
        self.events.append(self._event())

    def ms(self):
        torch.cuda.synchronize()
        return {n: a.elapsed_time(b) for n, a, b in zip(self.names, self.events, self.events[1:])}


def _measure(fn, repeats):
    """fn(mark) -> stats; -> (per-stage ms of every run, medians, host seconds of every run, the last stats)."""
    runs, host, stats = [], [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        marks, t0 = _Marks(), time.time()
        stats = fn(marks)
        runs.append(marks.ms())  # synchronises
        host.append(time.time() - t0)
    return runs, {k: float(np.median([r[k] for r in runs])) for k in runs[0]}, host, stats


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--params", default=os.path.join(REPO, "tests", "golden", "params_trained_l8_w256.npz"))
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target-faces", type=int, default=50000)
    ap.add_argument("--decimate-cells", type=int, default=64)
    ap.add_argument("--texels", type=int, default=texture.DEFAULT_TEXELS)
    ap.add_argument("--iso", type=float, default=mesh.DEFAULT_ISO)
    ap.add_argument("--quantile", type=float, default=0.9, help="the level where --iso lies above every density of the grid")
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--exports", type=int, default=2, help="textured exports of each kind, run alternately")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("decimate_report needs a GPU", file=sys.stderr)
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
    res, bounds = args.resolution, mesh.DEFAULT_BOUNDS
    report = {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "bounds": list(bounds), "resolution": res,
              "texels": args.texels, "mma": args.mma, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
              "note": "stage milliseconds from device events at the stage boundaries (search holds the probes' host reads); host_seconds: "
                      "the host's clock around the whole call, ending in a synchronise; export seconds as mesh.export_mesh reports them "
                      "(write: host clock).  The fixture is not a real scene: the cluster-cell footprint of the attribute query, any "
                      "effect on rendered appearance and the mesh quality against an edge-collapse simplifier are not measured"}
    with tempfile.TemporaryDirectory() as tmp, torch.cuda.device(dev):
        opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
        ckpt = trainer.save_checkpoint(trainer.checkpoint_path(tmp, 0), model, opt, 0)
        vol = mesh.density_grid(model.field, bounds, res)
        flat = vol.reshape(-1)
        if bool((flat >= args.iso).any()):
            iso, level = args.iso, "iso"
        else:
            iso = float(torch.quantile(flat[:: max(1, flat.numel() // (1 << 22))].double(), args.quantile))
            level = f"p{100 * args.quantile:g}"
        _, origin, spacing = mesh.grid_frame(bounds, res)
        surface = mesh.extract_surface(vol, iso, origin, spacing)
        del vol, flat
        report.update(level=iso, level_from=level, vertices_extracted=int(surface["positions"].shape[0]),
                      triangles_extracted=int(surface["triangles"].shape[0]))
        print(f"resolution {res}: level {iso:g} ({level}), {report['triangles_extracted']} triangles", flush=True)
        max_cells = res - 1

        def to_budget(mark):
            return decimate.decimate_to(surface, bounds, args.target_faces, max_cells, mark)[1]

        def to_cells(mark):
            return decimate.decimate(surface, bounds, args.decimate_cells, mark)["stats"]

        for name, fn in (("target_faces", to_budget), ("decimate_cells", to_cells)):
            fn(None)  # warm-up: code objects, torch's sort, the allocator
            runs, med, host, stats = _measure(fn, args.repeats)
            report[name] = {"stage_ms": runs, "median_stage_ms": med, "median_total_ms": float(np.median([sum(r.values()) for r in runs])),
                            "host_seconds": host, "median_host_seconds": float(np.median(host)), "stats": stats}
            print(name, json.dumps(report[name]["median_stage_ms"]), json.dumps(stats), flush=True)
        del surface
        # the whole textured export, without and with the budget, alternately
        mesh.export_mesh(ckpt, os.path.join(tmp, "warm.obj"), resolution=24, iso=iso, mma=args.mma, texture=True, texels=args.texels,
                         target_faces=100)  # warm-up
        exports = {"plain": [], "target_faces": []}
        for i in range(args.exports):
            for kind, kw in (("plain", {}), ("target_faces", {"target_faces": args.target_faces})):
                out = os.path.join(tmp, f"{kind}{i}.obj")
                t0 = time.time()
                r = mesh.export_mesh(ckpt, out, resolution=res, iso=iso, mma=args.mma, texture=True, texels=args.texels, **kw)
                run = {"wall_seconds": time.time() - t0, "seconds": r["seconds"], "vertices": r["vertices"], "triangles": r["triangles"],
                       "texture_size": r["texture_size"], "live_texels": r["live_texels"], "min_footprint": r["min_footprint"],
                       "file_bytes": {k: os.path.getsize(p) for k, p in r["files"].items()}}
                if "decimate" in r:
                    run["decimate"] = r["decimate"]
                exports[kind].append(run)
                print(f"export {kind} {i}: {r['triangles']} triangles, {r['texture_size']}^2 texels, wall {run['wall_seconds']:.2f} s, "
                      f"seconds {json.dumps(r['seconds'])}", flush=True)
                for p in r["files"].values():
                    os.remove(p)
        report["textured_export"] = exports
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report)[:2000])
    return 0


if __name__ == "__main__":
    sys.exit(main())
