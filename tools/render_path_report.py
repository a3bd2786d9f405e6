"""Where the time of a rendered frame goes (profiles/render_path.json).

    python tools/render_path_report.py --out profiles/render_path.json [--params tests/golden/params_trained_l8_w256.npz]
                                       [--size 800] [--frames 4] [--chunks 1024 4096] [--mma f32]

Builds the model the parameter fixture belongs to (the procedural scene's trained weights) and renders a short orbit with
render.render_path at every chunk size, PNG encoding of each frame included, as the `render` command does it.  Recorded per
chunk size and frame: the milliseconds between the device events render_path records (rays, field evaluation = the model's
chunked eval render, the visualisation launches, the copy to the host), the host milliseconds of the PNG encode, and for the
whole run the wall time per frame and rays per second.  The first frame of the first run carries the one-time work (weight
packing, the colour table, stream creation); it is recorded like the others and left out of the means.  Recorded values; no
threshold."""
import argparse
import io
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
from reflect_sampling_nerf_amd import render, trainer  # noqa: E402

STAGES = ("rays", "field", "visualize", "copy")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    ap.add_argument("--params", default=os.path.join(REPO, "tests", "golden", "params_trained_l8_w256.npz"))
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--mma", default="f32")
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--elevation", type=float, default=30.0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("render_path_report needs a GPU", file=sys.stderr)
        return 2
    from PIL import Image

    pz = np.load(args.params, allow_pickle=False)
    state = {k: torch.from_numpy(pz[k]) for k in pz.files}
    layers = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("mlp_base.layers."))
    width = int(state["mlp_base.layers.0.weight"].shape[0])
    model = trainer.make_model(pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=layers, base_mlp_layer_width=width))
    model.field.load_state_dict(state, strict=True)
    model.to("cuda:0").eval()
    model.field.set_mma_mode(args.mma)
    H = W = args.size
    intr = render.pinhole(W, H, 0.6911112070083618)  # camera_angle_x of the Blender synthetic scenes
    poses = render.orbit_path(args.frames, (0.0, 0.0, 0.0), args.radius, args.elevation)
    channels = render.DEFAULT_CHANNELS
    report = {"params": os.path.relpath(args.params, REPO), "network": [layers, width], "mma": args.mma, "size": [W, H],
              "frames": args.frames, "channels": list(channels), "orbit": {"radius": args.radius, "elevation_deg": args.elevation},
              "device": torch.cuda.get_device_name(0),
              "note": "milliseconds per frame between device events (rays / field / visualize / copy) and on the host (encode: PNG "
                      "into memory); means leave out frame 0 of each run", "runs": []}
    for chunk in args.chunks:
        model.config.eval_num_rays_per_chunk = int(chunk)
        events, encode_ms = [], []

        def encode(i, arr):
            t0 = time.perf_counter()
            Image.fromarray(arr).save(io.BytesIO(), format="PNG")
            encode_ms.append((time.perf_counter() - t0) * 1e3)

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        render.render_path(model, poses, H, W, *intr, channels, None, encode, stage_events=events)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        frames = [{**{s: ev[k].elapsed_time(ev[k + 1]) for k, s in enumerate(STAGES)}, "encode": encode_ms[i]} for i, ev in enumerate(events)]
        rest = frames[1:] or frames
        report["runs"].append({"chunk": int(chunk), "per_frame_ms": frames,
                               "mean_ms": {s: float(np.mean([f[s] for f in rest])) for s in (*STAGES, "encode")},
                               "wall_seconds_per_frame": wall / args.frames, "rays_per_second": args.frames * H * W / wall})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
