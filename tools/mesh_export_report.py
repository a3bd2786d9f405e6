"""Per-stage times of one mesh export (profiles/mesh_export.json).

    python tools/mesh_export_report.py --out profiles/mesh_export.json [--params tests/golden/params_trained_l8_w256.npz]
                                       [--resolution 256] [--iso 10] [--repeats 3]

Builds the model the parameter fixture belongs to, writes it as a trainer checkpoint into a temporary directory and runs
mesh.export_mesh on it: once at a small resolution (first launches, weight packing, allocator), then `repeats` times at the
asked resolution.  Recorded per run: the seconds of each stage (grid evaluation, count, emit -- which includes the host's
read-back of the two counts -- attributes, file write) from device events, the counts, and once the density's quantiles,
so that the iso level can be read against them.  When the default level gives no surface on this model, the runs are
repeated at the density's 90th percentile and both are recorded.  Recorded values; no threshold."""
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
from reflect_sampling_nerf_amd import _abi, mesh, trainer  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--params", default=os.path.join(REPO, "tests", "golden", "params_trained_l8_w256.npz"))
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--iso", type=float, default=mesh.DEFAULT_ISO)
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("mesh_export_report needs a GPU", file=sys.stderr)
        return 2
    pz = np.load(args.params, allow_pickle=False)
    state = {k: torch.from_numpy(pz[k]) for k in pz.files}
    layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("mlp_base.layers."))
    width = int(state["mlp_base.layers.0.weight"].shape[0])
    model = trainer.make_model(pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=layers, base_mlp_layer_width=width))
    model.field.load_state_dict(state, strict=True)
    model.to("cuda:0").eval()
    report = {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "resolution": args.resolution,
              "mma": args.mma, "bounds": list(mesh.DEFAULT_BOUNDS), "device": torch.cuda.get_device_name(0),
              "workspace_bytes": int(_abi.load_library().rsn_mesh_workspace_bytes(*[args.resolution] * 3)),
              "note": "seconds per stage from device events; `emit` includes the host read-back of the two counts"}
    with tempfile.TemporaryDirectory() as tmp:
        opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
        ckpt = trainer.save_checkpoint(trainer.checkpoint_path(tmp, 0), model, opt, 0)
        ply = os.path.join(tmp, "mesh.ply")
        mesh.export_mesh(ckpt, ply, resolution=32, iso=args.iso, mma=args.mma)  # warm-up
        vol = mesh.density_grid(model.field, mesh.DEFAULT_BOUNDS, args.resolution, mma=args.mma)
        q = torch.quantile(vol.reshape(-1)[:: max(1, vol.numel() // (1 << 22))].double(),
                           torch.tensor([0.0, 0.5, 0.9, 0.99, 0.999, 1.0], dtype=torch.float64, device=vol.device))
        report["sigma_quantiles"] = dict(zip(("min", "p50", "p90", "p99", "p99.9", "max"), [float(x) for x in q]))
        del vol
        levels = [("default", args.iso)]
        for name, iso in levels:
            runs = []
            for _ in range(max(1, args.repeats)):
                res = mesh.export_mesh(ckpt, ply, resolution=args.resolution, iso=iso, mma=args.mma)
                runs.append({"vertices": res["vertices"], "triangles": res["triangles"], "seconds": res["seconds"],
                             "ply_bytes": os.path.getsize(ply)})
            report[f"iso_{name}"] = {"iso": iso, "runs": runs}
            if name == "default" and runs[-1]["triangles"] == 0:
                levels.append(("p90", report["sigma_quantiles"]["p90"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
