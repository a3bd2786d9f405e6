"""Standalone training and evaluation on Blender-format scenes and nerfstudio-format captures, without nerfstudio.

    python -m reflect_sampling_nerf_amd.trainer train --data DIR --out DIR [--steps N] [--rays 1024] [--mma f32|bf16x6|bf16] [--resume FILE|DIR] [--max-grad-norm X] [--skip-nonfinite] [--multiscale L] [--distortion-loss X [--distortion-loss-coarse Y]] [--depth-loss X [--depth-loss-coarse Y] [--depth-sigma S] [--depth-unit-scale U] [--depth-euclidean]]
    python -m reflect_sampling_nerf_amd.trainer eval --data DIR --ckpt FILE|DIR [--split test] [--out metrics.json] [--multiscale L] [--normals [--normals-suffix _normal] [--normals-space world|camera]] [--depth [--depth-unit-scale U] [--depth-euclidean]]
    python -m reflect_sampling_nerf_amd.trainer export-mesh --ckpt FILE|DIR --out mesh.ply [--resolution N] [--iso S]
    python -m reflect_sampling_nerf_amd.trainer export-mesh --method tsdf --ckpt FILE|DIR --out mesh.ply --data DIR | --poses FILE.json [--max-views N] [--downscale K] [--trunc T]
    python -m reflect_sampling_nerf_amd.trainer export-mesh ... --out mesh.obj --texture [--texels 8] [--min-footprint F]
    python -m reflect_sampling_nerf_amd.trainer export-mesh ... [--decimate-cells N | --target-faces N]
    python -m reflect_sampling_nerf_amd.trainer export-pointcloud --ckpt FILE|DIR --out cloud.ply --data DIR | --poses FILE.json [--max-views N] [--downscale K] [--resolution 512] [--min-accumulation 0.5] [--edge 0.05 | --no-edge] [--no-thin]
    python -m reflect_sampling_nerf_amd.trainer render --ckpt FILE|DIR --out DIR [--data DIR | --poses FILE.json | --width W --height H --fov-x DEG --radius R]
    (train, eval, render, on a nerfstudio-format capture: [--data-format auto|blender|nerfstudio] [--orientation up|none] [--center poses|none] [--no-auto-scale] [--train-split-fraction F] [--eval-mode fraction|all]; train: [--near N --far F] [--primary-spacing uniform|reciprocal [--primary-tan T]])
    (eval and render: [--skip-empty | --skip-empty-samples [--occupancy-resolution N] [--occupancy-sigma S] [--occupancy-dilate D] [--occupancy-bounds X0 Y0 Z0 X1 Y1 Z1]])

`train` is the reference's `ns-train reflect-sampling-nerf --data DIR` loop on this package's own pieces: the reference
Model config (ReflectSamplingNeRFModelConfig defaults), RayDataManager batches (1024 rays, reflect_sampling_nerf_config.py:36-41),
parallel.train_step (50-step loss warm-up included) and FusedRAdam with the reference's schedule (config.py:50-53).  Checkpoints
use nerfstudio's layout (step-{step:09d}.ckpt holding step / pipeline / optimizers / scalers).  `eval` renders held-out
views in the reference's 1024-ray chunks and writes an ns-eval-shaped JSON: psnr, coarse_psnr, fine_psnr
(get_image_metrics_and_images) and fine_ssim (metrics.ssim of the clipped mid_reflect_fine render, model.py:468-479).
fine_lpips is not computed: it needs pretrained network weights that are not part of this package.

`train --resume PATH` continues a run from a step-*.ckpt (or from the newest one of a run directory): model, FusedRAdam moments and
step count, and -- from the trainer's own checkpoints, which carry a fifth key `rsn_run` -- the run's settings and both torch
generators.  `--steps` stays the total: a checkpoint of step k continues at k + 1 and writes the file names the uninterrupted run
would.  With --deterministic the continuation has the uninterrupted run's bits; in the default mode the first resumed step's forward
pass and loss do, and later steps differ as two uninterrupted default runs differ (the order of the weight-gradient atomics).  A
checkpoint without `rsn_run` (the reference's ns-train, or an older trainer) continues with the arguments given and a fresh jitter
stream.  Multi-GPU training is not offered here.

`train --max-grad-norm X` clips the global gradient norm to X before every optimiser step (nerfstudio's OptimizerConfig.max_norm),
and `--skip-nonfinite` leaves parameters and moments untouched on a step whose gradients hold an inf or a NaN (what torch's
GradScaler does for `ns-train` under mixed precision); both are off by default and decided on the device (FusedRAdam).  A guarded
run's log lines carry the gradient norm, the clip factor and the number of skipped steps, and the first line after a skip names the
parameters whose gradients were not finite.  Both settings are recorded in the checkpoint and come back with --resume.

`--data DIR` with a transforms.json in it is a nerfstudio-format capture (ns-process-data's output; transforms_train.json: a Blender-
format scene; --data-format overrides): per-frame or global fl_x fl_y cx cy w h and OpenCV coefficients k1 k2 k3 p1 p2, JPEG or PNG
frames named with their extension, sorted by name (data.load_nerfstudio_split).  The poses are normalised as nerfstudio does --
--orientation up rotates the cameras' mean up axis onto +z, --center poses moves their mean position to the origin, and the
translations are scaled so that the largest component is --scale-factor (--no-auto-scale: times --scale-factor alone) -- over all
frames, and then split: ceil(N F) evenly spaced frames train, the others are held out for `eval` (--eval-mode all: every frame does
both).  Distorted rays are made on the device (include/rsn.h, "captures").  `train` records how it read the capture, and the transform
and scale it applied, in the checkpoint and in OUT/dataparser_transforms.json (nerfstudio's file); --resume, `eval` and `render --data`
take them from there unless told otherwise (`--center-poses` is their name for train's --center), so a checkpoint is evaluated and
rendered in the frame it was trained in.  `render --data` on a capture renders the file's frames through their own cameras; an orbit
(--path orbit) goes through the first camera's pinhole part.  A capture's primary rays default to --near 0.05 --far 256
--primary-spacing reciprocal --primary-tan 1 (s(t) = t / (1/T + t); far 256 is the far of the model's own reflected rays): starting
points that have NOT been measured on a scene.  The four flags work on a Blender-format scene too, whose defaults stay 2, 6 and
uniform with nothing recorded; what is recorded, every tool that opens the checkpoint applies.  A frame's mask_path is read (first
channel non-zero = live): a masked pixel is never drawn into a training batch, and `eval` adds psnr_masked, the PSNR over the live
pixels, to the whole-image scores.  OPENCV_FISHEYE cameras (k1 .. k4) cast their rays through the equidistant model on the device.
--downscale-factor K reads images_K/ and masks_K/ beside images/ with the intrinsics over K (recorded when K != 1; nothing is
resampled).  Images of differing sizes and equirectangular cameras are errors that name the frame; the TSDF and point-cloud exports
take a capture only when all its cameras are equal and undistorted.

`train --multiscale L` and `eval --multiscale L` are mip-NeRF's multi-scale protocol (Barron et al. 2021) for L = 2 .. 5: every view
also exists at 1/2 .. 1/2^(L-1) of its size, as box averages of the white-blended pixels built once on the device (data.py).  Training
draws each ray's scale with probability 1/L -- in expectation mip-NeRF's objective, which draws uniformly over the pixels of all
scales and weights a ray's loss by its pixel's area: the same objective by importance sampling, with the losses untouched.  `eval`
renders and scores every view at every scale against the pyramid's ground truth: the JSON's psnr_x1, psnr_x2, psnr_x4, ... (and so on
for every metric) are the means over the views at one scale, the plain keys the mean of those per-scale means.  The image size must
be divisible by 2^(L-1), and `eval` needs the smallest scale to be at least 11 x 11 (the SSIM window).  The setting is recorded in the
checkpoint when it is above 1 and comes back with --resume; the default, 1, is the single-scale run with the launches, bytes and
checkpoint keys it always had.

`train --distortion-loss X` adds the distortion loss of mip-NeRF 360 (Barron et al. 2022, eq. 15; nerfstudio's distortion_loss) of
the fine level's compositing weights to the objective, X times its mean over the batch's rays, and `--distortion-loss-coarse Y` the
coarse level's: the term pulls a ray's weights together into one compact interval, on the samplers' normalised spacing bins
(include/rsn.h: rsn_distortion_forward / _backward).  mip-NeRF 360 uses 0.01 and nerfacto 0.002; neither value has been measured on
this method.  The reflect levels never get the term (their weights are detached).  Both are off by default, and the default run has
the launches, bytes and checkpoint keys it always had; a coefficient that is set is recorded in the checkpoint and comes back with
--resume.

`train --depth-loss X` supervises a capture with depth maps -- frames with a depth_file_path, as `ns-process-data polycam --use-depth`
and `record3d` write them: 16-bit PNGs or .npy arrays, --depth-unit-scale U (0.001, millimetres) times the pose scale -- with the
DS-NeRF depth term (Deng et al. 2022; include/rsn.h: rsn_depth_loss_forward / _backward) of the fine level, X times its mean over the
batch's rays; `--depth-loss-coarse Y` adds the coarse level's.  --depth-sigma S is the term's standard deviation around the measured
depth in scene units (0.1); --depth-euclidean says that the files hold distances along the ray, not z-depths (fisheye cameras need
that).  X, Y and S are starting points: no scene has been measured.  With --multiscale only the full-resolution rays are supervised
(the pyramid builds no depth levels: a design rule).  The depth files are read only when a depth flag asks for them; what is set is
recorded in the checkpoint and comes back with --resume, and the default run has the launches, bytes and checkpoint keys it always
had.  `eval --depth` scores every view's depth_fine against the same maps on the device (metrics.depth_error): the JSON gains
depth_mae and depth_rmse in scene units with their _std, depth_valid, the share of supervised pixels, and the per-image values.

`eval --normals` scores the geometry as the Ref-NeRF family's tables do: the scene's ground-truth normal maps (FILE_normal.png beside
every FILE.png, multinerf's naming of the Shiny Blender scenes; --normals-suffix names another) are read with the split, and every
view's composited predicted normal -- sum_s w_s n_s of the fine level, what the reflected rays start from -- is compared with them on
the device (metrics.normal_error).  The JSON gains normal_mae, the mean over the views of the alpha-weighted mean angular error in
degrees (multinerf's compute_normal_mae), and alpha_mae, the mean absolute difference between the fine accumulation and the ground-
truth alpha, each with its _std, and normal_mae_views, the number of views that had a pixel to score.  The maps are taken as world-
space normals, which is what Shiny Blender ships; --normals-space camera rotates them by each view's pose first.  With --multiscale
only the full-resolution renders are scored this way.  The analytic (density-gradient) normals are not scored: the eval path does
not form them.  Off by default, and the default eval has the launches, keys and bytes it always had.

`export-mesh` takes the learnt geometry out of a checkpoint: the field's density on a regular grid, its iso-surface extracted on
the device, and the diffuse colour, tint, roughness and predicted normal of the field at every surface vertex, as a binary PLY
(mesh.py).  The default level, sigma = 10, is a starting point that has not been measured against a scene.
With `--method tsdf` the surface is instead the one the model itself renders: its median depth is rendered from the cameras of
--data's split or of --poses (every one, or --max-views evenly spaced ones, at 1/--downscale of their size), the depth maps are
fused into a truncated signed distance volume on the same grid, and its zero level is extracted, the part between observed grid
vertices kept, and coloured as before.  No density level is involved.  The defaults, a truncation of 4 grid spacings and
--min-weight 1, are starting points from an experiment on analytic depth maps of a sphere, not measured on a scene.
With `--texture` either method writes a textured OBJ instead of the PLY (texture.py): NAME.obj, NAME.mtl and four PNG maps -- diffuse
colour, tint, roughness and the object-space predicted normal -- in which every pair of triangles owns a square of --texels x --texels
texels and the field is queried once per texel, with a footprint no smaller than --min-footprint.  The maps are the field's material
decomposition, not a rendered colour.  The defaults, 8 texels and the largest grid spacing / 8, are starting points, not measured on
a scene.
With `--decimate-cells N` or `--target-faces N` either method reduces the extracted mesh by vertex clustering before it is coloured
or textured (decimate.py): N cluster cells per axis over --bounds, or the cell count that leaves at most N triangles.  The merged
vertices are queried with the cluster cell as footprint; that rule, the effect on appearance and the quality against an edge-collapse
simplifier have not been measured.  Without the two flags nothing is reduced.

`export-pointcloud` writes the surface the model renders as points (pointcloud.py): one point per pixel of the depth maps rendered
from the cameras of --data's split or of --poses, origin + depth_fine * direction -- where the model starts its reflected rays --, for
the pixels whose accumulation reaches --min-accumulation, whose depth is no silhouette edge (--edge) and whose point lies in --bounds;
a grid of --resolution cells per axis keeps one point per cell (--no-thin: all).  The file is a PLY with the vertex layout of
export-mesh and no face element; a point's colour is the field's diffuse colour there, not a rendered pixel.  The defaults (512 cells
per axis, accumulation 0.5, edge 0.05) are starting points, not measured on a scene.

`render` draws a checkpoint from viewpoints of the user's choosing (render.py): an orbit around a centre, or the poses of a
transforms-format file, optionally with poses interpolated in between.  Every frame is a PNG panel of the chosen channels side by
side -- the final colour, the direct pass, diffuse colour, tint, roughness, predicted normals, turbo-coloured depth, accumulation,
the reflection mask -- or, with --tiles, one PNG per channel; frames.json records the cameras.  There is no video encoder here:
the frames are the product.

`eval` and `render` take `--skip-empty`: an occupancy grid of the field's density is built once (occupancy.py), and the rays whose
[near, far] segment crosses no occupied cell are not evaluated; they get the white background.  The grid's defaults (sigma 0.01,
one cell of dilation) are starting points from one experiment on a briefly trained field, not measured against a scene.  The
output JSON then carries an "occupancy" entry: the settings, the box, the occupied share of cells and the culled share of rays.
`--skip-empty-samples` implies it and goes one step further: on the rays that remain, the field is evaluated only on the samples
whose interval crosses an occupied cell (or whose cone is wider than the grid's dilation margin -- a design rule, not a measured
one); the others get zero density.  The "occupancy" entry then also holds "samples": per level, the sample slots seen and the live
ones.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Callable, Optional

import numpy as np
import torch

from .checkpoint import (COEFFICIENTS, PRIMARY_SPACINGS, RAY_KEYS, RUN_SETTINGS, RUN_STATE_KEY, RUN_STATE_VERSION,  # noqa: F401 (re-exported)
                         _load_pipeline, _Pipeline, checkpoint_path, config_for_checkpoint, config_with_planes, latest_checkpoint,
                         load_checkpoint, make_model, make_run_state, open_checkpoint, read_run_state, recorded_settings,
                         resolve_checkpoint, save_checkpoint, set_primary_sampler)

METHOD_NAME = "reflect-sampling-nerf"
MMA_CHOICES = ("f32", "bf16x6", "bf16")
EVAL_CHUNK = 1024  # reflect_sampling_nerf_config.py:41 eval_num_rays_per_chunk
RUN_DEFAULTS = {k: s.default for k, s in RUN_SETTINGS.items() if s.default is not None}  # what a fresh run gets when not told (the others: None)
DEFAULT_NORMALS_SUFFIX = "_normal"  # multinerf / Shiny Blender: r_0.png beside r_0_normal.png
NORMALS_SPACES = ("world", "camera")
# A capture (a nerfstudio-format transforms.json): how it is read when nothing says otherwise (nerfstudio's NerfstudioDataParserConfig) ...
CAPTURE_DATA_DEFAULTS = {"orientation": "up", "center": "poses", "auto_scale": True, "scale_factor": 1.0, "train_split_fraction": 0.9,
                         "eval_mode": "fraction"}
# ... and how its primary rays are cast: far 256 is the far of the model's own reflected rays, reciprocal spacing puts the samples
# where an unbounded scene needs them.  Starting points that have NOT been measured on a scene.  Blender-format scenes keep the
# model's own 2 .. 6 with uniform spacing.
CAPTURE_RAY_DEFAULTS = {"near": 0.05, "far": 256.0, "primary_spacing": "reciprocal", "primary_tan": 1.0}


class _NotGiven(float):
    """The default of --scale-factor: 1.0 to everything that computes with it, and recognisable as "the user typed nothing", so that a
    capture's scale_factor can come from the checkpoint's record."""


SCALE_NOT_GIVEN = _NotGiven(1.0)
LPIPS_NOTE = "fine_lpips not computed: LPIPS needs pretrained network weights that are not shipped with this package"


OCCUPANCY_SUBFLAGS = ("occupancy_resolution", "occupancy_sigma", "occupancy_dilate", "occupancy_bounds")


def _flags_need(ap: argparse.ArgumentParser, args, names, needed: str, more=()) -> None:
    """The error for flags that have no meaning without `needed`: those of `names` (attributes of args; --like-this on the command
    line) that were given, and `more` (flag texts the caller found given by a test of its own)."""
    stray = ["--" + n.replace("_", "-") for n in names if getattr(args, n, None) is not None] + list(more)
    if stray:
        ap.error(f"{args.command}: {' '.join(stray)} need(s) {needed}")


def _check_box(ap: argparse.ArgumentParser, args, flag: str, b) -> None:
    if b is not None and not (all(math.isfinite(x) for x in b) and all(b[3 + a] > b[a] for a in range(3))):
        ap.error(f"{args.command}: {flag} needs X0 Y0 Z0 X1 Y1 Z1 with every upper bound above its lower one")


def _add_occupancy_flags(p: argparse.ArgumentParser) -> None:
    from .occupancy import DEFAULT_DILATE, DEFAULT_RESOLUTION, DEFAULT_SIGMA

    p.add_argument("--skip-empty", action="store_true",
                   help="cull the rays that cross no occupied cell of an occupancy grid built from the field (they get the white background)")
    p.add_argument("--skip-empty-samples", action="store_true",
                   help="implies --skip-empty; on the remaining rays, evaluate the field only on the samples whose interval crosses an "
                        "occupied cell or whose cone is wider than the grid's dilation margin (a design rule, not measured against any scene)")
    p.add_argument("--occupancy-resolution", type=int, default=None, metavar="N", help=f"grid vertices per axis (default {DEFAULT_RESOLUTION})")
    p.add_argument("--occupancy-sigma", type=float, default=None, metavar="S",
                   help=f"a cell is occupied when a corner has density >= S (default {DEFAULT_SIGMA:g}: a starting point from one experiment "
                        "on a field trained for 2000 steps, not measured against any scene; pick it per scene)")
    p.add_argument("--occupancy-dilate", type=int, choices=(0, 1, 2), default=None, metavar="D",
                   help=f"grow the occupied cells by D cells, 0..2 (default {DEFAULT_DILATE}: a starting point from the same experiment)")
    p.add_argument("--occupancy-bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="box of the grid (default: a box around the [near, far] segments of the cameras' rays); what it does not cover counts as occupied")


def resolve_occupancy_args(ap: argparse.ArgumentParser, args) -> Optional[dict]:
    """The occupancy settings of an `eval` / `render` command line: None without --skip-empty and --skip-empty-samples (the sub-flags
    are an error then), else {"resolution", "sigma", "dilate", "bounds" (None: from the cameras)}, with "samples": True added by
    --skip-empty-samples (absent means False: --skip-empty alone resolves to what it always did)."""
    from .occupancy import DEFAULT_DILATE, DEFAULT_RESOLUTION, DEFAULT_SIGMA

    samples = bool(getattr(args, "skip_empty_samples", False))
    if not (getattr(args, "skip_empty", False) or samples):
        _flags_need(ap, args, OCCUPANCY_SUBFLAGS, "--skip-empty")
        return None
    res = DEFAULT_RESOLUTION if args.occupancy_resolution is None else args.occupancy_resolution
    sigma = DEFAULT_SIGMA if args.occupancy_sigma is None else args.occupancy_sigma
    if res < 2 or res ** 3 > 2 ** 27:
        ap.error(f"{args.command}: --occupancy-resolution {res}: need 2 <= N <= 512")
    if not math.isfinite(sigma):
        ap.error(f"{args.command}: --occupancy-sigma {sigma}: need a finite value")
    b = args.occupancy_bounds
    _check_box(ap, args, "--occupancy-bounds", b)
    settings = {"resolution": int(res), "sigma": float(sigma), "dilate": DEFAULT_DILATE if args.occupancy_dilate is None else args.occupancy_dilate,
                "bounds": None if b is None else tuple(float(x) for x in b)}
    if samples:
        settings["samples"] = True
    return settings


def _add_data_flags(p: argparse.ArgumentParser, train: bool) -> None:
    """--data-format and how a capture is read.  Every default is None: "not given", so that a checkpoint's own record decides."""
    from .data import CENTERS, DATA_FORMATS, EVAL_MODES, ORIENTATIONS

    whose = "" if train else "; default: the checkpoint's"
    p.add_argument("--data-format", choices=DATA_FORMATS, default="auto",
                   help="auto: a directory with transforms.json is a nerfstudio-format capture, one with transforms_train.json a Blender-format scene")
    p.add_argument("--orientation", choices=ORIENTATIONS, default=None,
                   help=f"capture: rotate the poses so that the cameras' mean up axis becomes +z (default up{whose})")
    p.add_argument("--center" if train else "--center-poses", dest="center_poses", choices=CENTERS, default=None,  # render has an orbit --center
                   help=f"capture: move the mean camera position to the origin (default poses{whose})")
    p.add_argument("--no-auto-scale", action="store_true", default=None,
                   help="capture: do not scale the poses so that the largest translation component is --scale-factor")
    p.add_argument("--train-split-fraction", type=float, default=None, metavar="F",
                   help=f"capture: the share of the frames, evenly spaced, that is trained on; the others are held out (default 0.9{whose})")
    p.add_argument("--eval-mode", choices=EVAL_MODES, default=None,
                   help=f"capture: fraction, or all: train and evaluate on every frame (default fraction{whose})")
    p.add_argument("--downscale-factor", type=_downscale_factor, default=None, metavar="K",
                   help="capture: read images_K/ (and masks_K/) beside images/, as ns-process-data writes them, with the intrinsics "
                        f"over K; nothing is resampled (default 1{whose})")


def _downscale_factor(text: str) -> int:
    try:
        k = int(text)
    except ValueError:
        k = 0
    if k < 1:
        raise argparse.ArgumentTypeError(f"{text!r}: an integer >= 1")
    return k


def build_parser(run_defaults: bool = True) -> argparse.ArgumentParser:
    """run_defaults=False: --rays / --mma / --seed parse to None when absent, so that `main` can tell "not given" (a resumed run then
    takes the checkpoint's value) from a value typed by the user."""
    dflt = RUN_DEFAULTS if run_defaults else dict.fromkeys(RUN_DEFAULTS)
    ap = argparse.ArgumentParser(prog="python -m reflect_sampling_nerf_amd.trainer", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", help="train on the train split of a Blender-format scene or of a nerfstudio-format capture")
    tr.add_argument("--data", required=True, help="scene directory with transforms_train.json (Blender format) or transforms.json (a capture)")
    tr.add_argument("--out", required=True, help="directory for step-*.ckpt")
    tr.add_argument("--steps", type=int, default=100000, help="training iterations (reference max_num_iterations)")
    tr.add_argument("--rays", type=int, default=dflt["rays"], help="rays per batch (default 1024)")
    tr.add_argument("--mma", choices=MMA_CHOICES, default=dflt["mma"],
                    help="matrix-core arithmetic of the field kernels (default f32)")
    tr.add_argument("--save-every", type=int, default=1000, help="checkpoint interval in steps")
    tr.add_argument("--log-every", type=int, default=100, help="loss read-back interval in steps (0: never)")
    tr.add_argument("--seed", type=int, default=dflt["seed"], help="model initialisation and ray sampling seed (default 0)")
    tr.add_argument("--deterministic", action="store_true",
                    help="bit-reproducible run: weight gradients reduced in a fixed order (slower flush, one 68 MB workspace)")
    tr.add_argument("--scale-factor", type=float, default=SCALE_NOT_GIVEN,
                    help="BlenderDataParser scale_factor (default 1); a capture: the dataparser's scale_factor, what the largest translation "
                         "component becomes under auto-scaling (default 1)")
    tr.add_argument("--max-grad-norm", type=float, default=None, metavar="X",
                    help="clip the global gradient norm to X before every optimiser step (default: no clipping)")
    tr.add_argument("--skip-nonfinite", action="store_true",
                    help="a step whose gradients hold an inf or a NaN changes no parameter and no optimiser moment")
    tr.add_argument("--multiscale", type=int, default=dflt["multiscale"], metavar="L",
                    help="draw the training rays from L scales of every image, 1, 1/2, ... 1/2^(L-1), each with probability 1/L "
                         "(1 to 5; default 1: full resolution only); the image size must be divisible by 2^(L-1)")
    tr.add_argument("--distortion-loss", type=float, default=None, metavar="X",
                    help="add X times the distortion loss of mip-NeRF 360 (eq. 15) of the fine level's weights to the objective: it pulls "
                         "each ray's weights into one compact interval.  mip-NeRF 360 uses 0.01 and nerfacto 0.002; neither value has "
                         "been measured on this method (default: off)")
    tr.add_argument("--distortion-loss-coarse", type=float, default=None, metavar="Y",
                    help="the same term on the coarse level's weights, times Y (default: off)")
    tr.add_argument("--depth-loss", type=float, default=None, metavar="X",
                    help="a capture with depth maps (depth_file_path, as ns-process-data polycam --use-depth / record3d write them): add X "
                         "times the DS-NeRF depth term of the fine level to the objective; it pulls each supervised ray's weight to its "
                         "measured depth.  A starting point, not measured on a scene (default: off)")
    tr.add_argument("--depth-loss-coarse", type=float, default=None, metavar="Y",
                    help="the same term on the coarse level, times Y (default: off)")
    tr.add_argument("--depth-sigma", type=float, default=None, metavar="S",
                    help="standard deviation of the depth term around the measured depth, in scene units (default 0.1: a starting point, "
                         "not measured on a scene)")
    tr.add_argument("--depth-unit-scale", type=float, default=None, metavar="U",
                    help="what one unit of a depth file is in the units of the poses (default 0.001: millimetres, nerfstudio's)")
    tr.add_argument("--depth-euclidean", action="store_true", default=None,
                    help="the depth files hold distances along the ray, not z-depths (needed for fisheye cameras)")
    _add_data_flags(tr, train=True)
    tr.add_argument("--near", type=float, default=None, metavar="N",
                    help="near plane of the primary rays (default: 2 for a Blender-format scene, 0.05 for a capture -- a starting point, not measured on a scene)")
    tr.add_argument("--far", type=float, default=None, metavar="F",
                    help="far plane of the primary rays (default: 6 for a Blender-format scene, 256 for a capture -- the far of the model's "
                         "own reflected rays; a starting point, not measured on a scene)")
    tr.add_argument("--primary-spacing", choices=PRIMARY_SPACINGS, default=None,
                    help="spacing of the primary rays' coarse samples: uniform in distance, or reciprocal, s(t) = t / (1/T + t) (default: uniform for "
                         "a Blender-format scene, reciprocal for a capture -- a starting point, not measured on a scene)")
    tr.add_argument("--primary-tan", type=float, default=None, metavar="T", help="T of the reciprocal spacing (default 1: a starting point, not measured)")
    tr.add_argument("--resume", default=None, metavar="PATH",
                    help="continue from this step-*.ckpt, or from the newest one in this run directory; --steps stays the total, and "
                         "--rays / --mma / --seed / --deterministic / --max-grad-norm / --skip-nonfinite / --multiscale / "
                         "--distortion-loss / --distortion-loss-coarse / --depth-loss / --depth-loss-coarse / --depth-sigma / "
                         "--depth-euclidean, the ray flags (--near / --far / --primary-spacing / --primary-tan) "
                         "and a capture's data flags come from the checkpoint unless given")
    ev = sub.add_parser("eval", help="score a checkpoint on held-out views")
    ev.add_argument("--data", required=True, help="scene directory with transforms_{split}.json (Blender format) or transforms.json (a capture)")
    ev.add_argument("--ckpt", required=True, help="step-*.ckpt written by `train` (or by ns-train), or a run directory (its newest)")
    ev.add_argument("--split", default="test")
    ev.add_argument("--max-images", type=int, default=None, help="score only the first N views")
    ev.add_argument("--out", default="metrics.json", help="output JSON")
    ev.add_argument("--save-images", default=None, help="directory for rendered ground truth | coarse | fine panels")
    ev.add_argument("--scale-factor", type=float, default=SCALE_NOT_GIVEN,
                    help="BlenderDataParser scale_factor (default 1); a capture: the dataparser's scale_factor (default: the checkpoint's)")
    _add_data_flags(ev, train=False)
    ev.add_argument("--multiscale", type=int, default=1, metavar="L",
                    help="score every view at L scales, 1, 1/2, ... 1/2^(L-1), against box-averaged ground truth (1 to 5; default 1); "
                         "the results gain KEY_x1, KEY_x2, ... per scale and the plain KEY becomes the mean of those")
    ev.add_argument("--normals", action="store_true",
                    help="also score the geometry against the scene's ground-truth normal maps: normal_mae, the alpha-weighted mean angular "
                         "error of the composited predicted normals in degrees, and alpha_mae, the accumulation against the alpha")
    ev.add_argument("--normals-suffix", default=None, metavar="S",
                    help=f"with --normals: a frame's normal map is file_path + S + .png (default {DEFAULT_NORMALS_SUFFIX}, the Shiny Blender naming)")
    ev.add_argument("--normals-space", choices=NORMALS_SPACES, default=None,
                    help="with --normals: the frame the normal maps are written in (default world, what Shiny Blender uses; camera: "
                         "OpenGL camera axes, rotated into the world by each view's pose)")
    ev.add_argument("--depth", action="store_true",
                    help="a capture with depth maps: also score depth_fine against them: depth_mae, depth_rmse (scene units) and "
                         "depth_valid, the share of supervised pixels")
    ev.add_argument("--depth-unit-scale", type=float, default=None, metavar="U",
                    help="with --depth: what one unit of a depth file is in the units of the poses (default: the checkpoint's, else 0.001)")
    ev.add_argument("--depth-euclidean", action="store_true", default=None,
                    help="with --depth: the depth files hold distances along the ray, not z-depths (default: the checkpoint's)")
    _add_occupancy_flags(ev)
    ex = sub.add_parser("export-mesh", help="write the iso-surface of a checkpoint's density as a coloured triangle mesh (PLY)")
    ex.add_argument("--ckpt", required=True, help="step-*.ckpt written by `train` (or by ns-train), or a run directory (its newest)")
    ex.add_argument("--out", required=True, help="output file (binary little-endian PLY)")
    ex.add_argument("--resolution", type=int, default=256, help="grid vertices per axis (default 256)")
    ex.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="box the grid spans (default -1.5 -1.5 -1.5 1.5 1.5 1.5, nerfstudio's Blender scene box)")
    ex.add_argument("--iso", type=float, default=None, metavar="S",
                    help="density level of the surface (default 10: a starting point, not measured against any scene; pick it per scene)")
    ex.add_argument("--mma", choices=MMA_CHOICES, default="f32", help="matrix-core arithmetic of the field kernels (default f32)")
    ex.add_argument("--chunk", type=int, default=None, help="points per field launch (default 262144)")
    ex.add_argument("--method", choices=("density", "tsdf"), default="density",
                    help="density: the iso-surface of the field's density at --iso (default); tsdf: the surface of the model's own depth "
                         "maps, rendered from the cameras of --data / --poses and fused into a truncated signed distance volume")
    ex.add_argument("--data", default=None, metavar="DIR", help="tsdf: scene directory; the cameras of transforms_{split}.json")
    ex.add_argument("--split", default="train", help="tsdf: the split of --data (default train)")
    ex.add_argument("--poses", default=None, metavar="FILE.json",
                    help="tsdf: transforms-format file with frames[].transform_matrix, camera_angle_x and w / h")
    ex.add_argument("--scale-factor", type=float, default=SCALE_NOT_GIVEN,
                    help="tsdf: scale of the translations read from --data / --poses (default 1; a capture: the checkpoint's)")
    _add_data_flags(ex, train=False)
    ex.add_argument("--max-views", type=int, default=None, metavar="N", help="tsdf: use N evenly spaced views of the file (default: all)")
    ex.add_argument("--downscale", type=int, default=1, metavar="K",
                    help="tsdf: render every depth map at 1/K of the cameras' size, intrinsics scaled alike (default 1)")
    ex.add_argument("--trunc", type=float, default=None, metavar="T",
                    help="tsdf: truncation distance in world units (default 4 x the largest grid spacing: a starting point from an "
                         "experiment on analytic depth maps of a sphere, not measured on a scene)")
    ex.add_argument("--min-weight", type=float, default=None, metavar="W",
                    help="tsdf: views a grid vertex needs to count as observed; surface between unobserved vertices is dropped "
                         "(default 1: a starting point from the same experiment, not measured on a scene)")
    ex.add_argument("--ray-chunk", type=int, default=None, metavar="R", help="tsdf: rays per chunk of the depth pass (default 4096)")
    ex.add_argument("--texture", action="store_true",
                    help="write a textured OBJ (--out NAME.obj, with NAME.mtl and four PNG maps: diffuse colour, tint, roughness, "
                         "object-space normal) instead of a PLY: the field sampled per texel of a per-triangle atlas")
    ex.add_argument("--texels", type=int, default=None, metavar="P",
                    help="texture: side of the square of texels a pair of triangles gets, at least 4 (default 8: a starting point, "
                         "not measured on a scene)")
    ex.add_argument("--min-footprint", type=float, default=None, metavar="F",
                    help="texture: the smallest footprint, in world units, a texel is queried with (default the largest grid spacing "
                         "/ 8: a starting point, not measured on a scene)")
    ex.add_argument("--decimate-cells", type=int, default=None, metavar="N",
                    help="reduce the extracted mesh by vertex clustering with N cluster cells per axis over --bounds (decimate.py); "
                         "the merged vertices' attributes are queried with the cluster cell as footprint (a design rule, not measured "
                         "on a scene).  No default: without this flag and --target-faces nothing is reduced")
    ex.add_argument("--target-faces", type=int, default=None, metavar="N",
                    help="reduce the extracted mesh by vertex clustering to at most N triangles: the cell count is searched from 2 up "
                         "to the grid's intervals per axis.  Excludes --decimate-cells")
    pc = sub.add_parser("export-pointcloud", help="write the surface a checkpoint's model renders as a coloured point cloud (PLY without faces)")
    pc.add_argument("--ckpt", required=True, help="step-*.ckpt written by `train` (or by ns-train), or a run directory (its newest)")
    pc.add_argument("--out", required=True, help="output file (binary little-endian PLY, vertex element only)")
    pc.add_argument("--data", default=None, metavar="DIR", help="scene directory; the cameras of transforms_{split}.json")
    pc.add_argument("--split", default="train", help="the split of --data (default train)")
    pc.add_argument("--poses", default=None, metavar="FILE.json",
                    help="transforms-format file with frames[].transform_matrix, camera_angle_x and w / h")
    pc.add_argument("--scale-factor", type=float, default=SCALE_NOT_GIVEN,
                    help="scale of the translations read from --data / --poses (default 1; a capture: the checkpoint's)")
    _add_data_flags(pc, train=False)
    pc.add_argument("--max-views", type=int, default=None, metavar="N", help="use N evenly spaced views of the file (default: all)")
    pc.add_argument("--downscale", type=int, default=1, metavar="K",
                    help="render every depth map at 1/K of the cameras' size, intrinsics scaled alike (default 1)")
    pc.add_argument("--resolution", type=int, default=512, metavar="N",
                    help="cells per axis of the grid that keeps one point per cell (default 512: a starting point, not measured on a scene)")
    pc.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="box the points must lie in (default -1.5 -1.5 -1.5 1.5 1.5 1.5, nerfstudio's Blender scene box)")
    pc.add_argument("--min-accumulation", type=float, default=0.5, metavar="A",
                    help="a pixel needs this accumulation (default 0.5: a starting point, not measured on a scene)")
    edge = pc.add_mutually_exclusive_group()
    edge.add_argument("--edge", type=float, default=0.05, metavar="E",
                      help="drop a pixel whose depth differs from a neighbour's by more than E times the smaller of the two "
                           "(default 0.05: a starting point, not measured on a scene)")
    edge.add_argument("--no-edge", action="store_true", help="keep the pixels on depth edges")
    pc.add_argument("--no-thin", action="store_true", help="keep every candidate pixel instead of one per grid cell")
    pc.add_argument("--mma", choices=MMA_CHOICES, default="f32", help="matrix-core arithmetic of the field kernels (default f32)")
    pc.add_argument("--ray-chunk", type=int, default=None, metavar="R", help="rays per chunk of the depth pass (default 4096)")
    pc.add_argument("--chunk", type=int, default=None, help="points per field launch of the attribute pass (default 262144)")
    from .render import CHANNELS, DEFAULT_CHANNELS, DEFAULT_CHUNK

    rn = sub.add_parser("render", help="render a camera path from a checkpoint as PNG panels of colour and material maps")
    rn.add_argument("--ckpt", required=True, help="step-*.ckpt written by `train` (or by ns-train), or a run directory (its newest)")
    rn.add_argument("--out", required=True, help="output directory: panel/0000.png ... (or <channel>/0000.png ... with --tiles), frames.json")
    rn.add_argument("--path", choices=("orbit", "poses"), default=None,
                    help="orbit around --center, or the poses of --poses / of --data's split (default: poses when --poses is given or --data "
                         "is a nerfstudio-format capture, whose frames are rendered through their own cameras; else orbit)")
    rn.add_argument("--frames", type=int, default=120, help="frames of an orbit (default 120)")
    rn.add_argument("--center", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"), help="orbit centre (default 0 0 0)")
    rn.add_argument("--radius", type=float, default=None,
                    help="orbit radius (default with --data: the mean distance of the split's cameras from --center)")
    rn.add_argument("--elevation", type=float, default=None, metavar="DEG",
                    help="orbit elevation above the xy-plane (default with --data: the mean elevation of the split's cameras; else 30)")
    rn.add_argument("--azimuth", type=float, default=0.0, metavar="DEG", help="azimuth of the orbit's first frame (default 0)")
    rn.add_argument("--poses", default=None, metavar="FILE.json", help="transforms-format file: frames[].transform_matrix, camera_angle_x, w / h")
    rn.add_argument("--data", default=None, metavar="DIR", help="scene directory: poses, field of view and image size of transforms_{split}.json")
    rn.add_argument("--split", default="test")
    rn.add_argument("--scale-factor", type=float, default=SCALE_NOT_GIVEN,
                    help="scale of the translations read from --poses / --data (default 1; a capture: the checkpoint's)")
    _add_data_flags(rn, train=False)
    rn.add_argument("--interpolate", type=int, default=0, metavar="K", help="poses inserted between consecutive ones of a poses path (default 0)")
    rn.add_argument("--width", type=int, default=None)
    rn.add_argument("--height", type=int, default=None)
    rn.add_argument("--fov-x", type=float, default=None, metavar="DEG", help="horizontal field of view in degrees")
    rn.add_argument("--channels", nargs="+", choices=tuple(CHANNELS), default=list(DEFAULT_CHANNELS), metavar="CHANNEL",
                    help="tiles of the panel, left to right: " + " ".join(CHANNELS) + " (default: " + " ".join(DEFAULT_CHANNELS) + ")")
    rn.add_argument("--depth-range", type=float, nargs=2, default=None, metavar=("NEAR", "FAR"),
                    help="range of the depth colour map (default: the model's collider planes)")
    rn.add_argument("--mma", choices=MMA_CHOICES, default="f32", help="matrix-core arithmetic of the field kernels (default f32)")
    rn.add_argument("--chunk", type=int, default=DEFAULT_CHUNK, help=f"rays per eval chunk (default {DEFAULT_CHUNK})")
    rn.add_argument("--tiles", action="store_true", help="one PNG per channel and frame instead of the tiled panel")
    _add_occupancy_flags(rn)
    return ap


def _scale_factor(args) -> float:
    return float(args.scale_factor)


CAPTURE_POSE_KEYS = ("orientation", "center", "auto_scale", "scale_factor")


def capture_load_args(args, recorded: Optional[dict] = None, depths: bool = False):
    """How a command line reads a capture -> (the keyword arguments of data.load_nerfstudio_split, the settings to record).  Each of
    CAPTURE_DATA_DEFAULTS' keys: the flag if given, else the record of the checkpoint's run (`recorded`: its rsn_run entry or None),
    else the default.  When the run recorded the transform and scale it applied and no flag that bears on the poses is given, exactly
    those are applied again: the checkpoint is trained on, evaluated and rendered in the frame it was trained in."""
    rec = (recorded or {}).get("data") or {}
    given = {"orientation": args.orientation, "center": args.center_poses, "auto_scale": False if args.no_auto_scale else None,
             "scale_factor": None if isinstance(args.scale_factor, _NotGiven) else float(args.scale_factor), "train_split_fraction": args.train_split_fraction, "eval_mode": args.eval_mode}
    settings = {k: given[k] if given[k] is not None else rec.get(k, dflt) for k, dflt in CAPTURE_DATA_DEFAULTS.items()}
    kwargs = dict(settings)
    # the downscale factor is passed on and recorded only when it is not 1: a capture without one keeps the record it always had
    asked = getattr(args, "downscale_factor", None)
    downscale = int(asked if asked is not None else rec.get("downscale_factor", 1))
    if downscale != 1:
        settings["downscale_factor"] = kwargs["downscale_factor"] = downscale
    if depths:  # the depth files are read, and their unit recorded, only when a depth flag (or the resumed run's record) asks
        asked = getattr(args, "depth_unit_scale", None)
        settings["depth_unit_scale"] = kwargs["depth_unit_scale"] = float(asked if asked is not None else rec.get("depth_unit_scale", 1e-3))
        kwargs["depths"] = True
    if rec.get("transform") is not None and all(given[k] is None for k in CAPTURE_POSE_KEYS):
        kwargs["applied"] = (rec["transform"], rec["scale"])
    return kwargs, settings


def capture_flags_given(args):
    """The capture-only flags a command line carries (for the error that says a Blender-format scene has no use for them)."""
    names = (("--orientation", "orientation"), ("--center", "center_poses"), ("--no-auto-scale", "no_auto_scale"),
             ("--train-split-fraction", "train_split_fraction"), ("--eval-mode", "eval_mode"), ("--downscale-factor", "downscale_factor"))
    return [flag for flag, attr in names if getattr(args, attr, None) is not None]


def load_scene(ap: argparse.ArgumentParser, args, split: str, recorded: Optional[dict] = None, pixels: bool = True, depths: bool = False,
               **blender):
    """The scene --data names -> (scene, the data settings to record: None for a Blender-format scene).  The format is detected
    (data.detect_data_format) unless --data-format says it.  blender: further arguments of load_blender_split (normals)."""
    from .data import detect_data_format, load_blender_split, load_nerfstudio_split

    try:
        fmt = detect_data_format(args.data, args.data_format)
    except FileNotFoundError as e:
        ap.error(f"{args.command}: {e}")
    if fmt == "blender":
        stray = capture_flags_given(args)
        if stray:
            ap.error(f"{args.command}: {' '.join(stray)} bear(s) on a nerfstudio-format capture; {args.data} is a Blender-format scene")
        if depths:
            ap.error(f"{args.command}: the depth flags need a nerfstudio-format capture with depth_file_path entries; {args.data} is a "
                     "Blender-format scene")
        return load_blender_split(args.data, split, _scale_factor(args), **blender), None
    if blender.get("normals"):
        ap.error(f"{args.command}: --normals needs a Blender-format scene with normal maps; {args.data} is a nerfstudio-format capture")
    kwargs, settings = capture_load_args(args, recorded, depths)
    try:  # masks and fisheye cameras are read where the file has them
        return load_nerfstudio_split(args.data, split, pixels=pixels, masks=True, fisheye=True, **kwargs), {"format": "nerfstudio", **settings}
    except FileNotFoundError as e:
        if "downscale_factor" not in kwargs:
            raise
        ap.error(f"{args.command}: --downscale-factor {kwargs['downscale_factor']}: {e}")


def resolve_render_args(ap: argparse.ArgumentParser, args) -> dict:
    """The cameras of a `render` command line: {"c2w" [F,3,4], "width", "height", "fx", "fy", "cx", "cy"}.  Host work only (JSON and
    one image header).  What the command line leaves open and no file settles is an argparse error that names the option."""
    from . import render

    if args.poses is not None and args.data is not None:
        ap.error("render: give --poses or --data, not both")
    capture, src = _camera_source(ap, args)
    if capture is not None:  # the cameras of the file's frames, in the frame the checkpoint was trained in
        src = {"c2w": capture.c2w, "width": capture.width, "height": capture.height,
               "camera_angle_x": 2.0 * math.atan(0.5 * capture.width / capture.fx), "file_paths": capture.file_paths}
    width = args.width if args.width is not None else (src or {}).get("width")
    height = args.height if args.height is not None else (src or {}).get("height")
    fov = math.radians(args.fov_x) if args.fov_x is not None else (src or {}).get("camera_angle_x")
    where = "" if src is None else " (the file gives none)"
    for name, v in (("--width", width), ("--height", height), ("--fov-x", fov)):
        if v is None:
            ap.error(f"render: {name} is required{where}: without --data / --poses all of --width --height --fov-x are")
    if width < 1 or height < 1 or not 0.0 < fov < math.pi:
        ap.error(f"render: --width {width} --height {height} --fov-x {math.degrees(fov):g}: need a positive size and 0 < fov < 180")
    path = args.path or ("poses" if args.poses is not None or capture is not None else "orbit")
    if path == "poses":
        if src is None:
            ap.error("render: --path poses needs --poses or --data")
        c2w = render.interpolate_path(src["c2w"], args.interpolate)
    else:
        radius, elevation = args.radius, args.elevation
        if args.data is not None:  # the split's own cameras say where a camera of this scene sits
            rel = src["c2w"][:, :, 3].astype(np.float64) - np.asarray(args.center, dtype=np.float64)
            dist = np.linalg.norm(rel, axis=1)
            if radius is None:
                radius = float(dist.mean())
            if elevation is None:
                elevation = float(np.degrees(np.arcsin(np.clip(rel[:, 2] / np.maximum(dist, 1e-30), -1.0, 1.0))).mean())
        if radius is None:
            ap.error("render: --radius is required for an orbit without --data")
        if elevation is None:
            elevation = 30.0
        try:
            c2w = render.orbit_path(args.frames, args.center, radius, elevation, args.azimuth)
        except ValueError as e:
            ap.error(f"render: {e}")
    if args.depth_range is not None and not args.depth_range[1] > args.depth_range[0]:
        ap.error("render: --depth-range needs NEAR < FAR")
    if args.chunk < 1:
        ap.error("render: --chunk must be >= 1")
    fx, fy, cx, cy = render.pinhole(width, height, fov)
    cameras = {"c2w": c2w, "width": int(width), "height": int(height), "fx": fx, "fy": fy, "cx": cx, "cy": cy}
    if capture is not None and path == "poses":  # the file's frames through their own cameras; an orbit: the first one's pinhole part
        if args.interpolate or args.width is not None or args.height is not None or args.fov_x is not None:
            ap.error("render: a capture's frames are rendered through their own cameras: --interpolate / --width / --height / --fov-x "
                     "do not apply (an orbit, --path orbit, takes them)")
        cameras.update(fx=capture.fx, fy=capture.fy, cx=capture.cx, cy=capture.cy, camera_table=capture.cameras)
    elif capture is not None and args.width is None and args.height is None and args.fov_x is None:
        cameras.update(fx=capture.fx, fy=capture.fy, cx=capture.cx, cy=capture.cy)  # an orbit: the first camera's pinhole part, no distortion
    return cameras


def _capture_cameras(ap: argparse.ArgumentParser, args):
    """The cameras of --data's split of a capture, read as the checkpoint's run read it (headers only, no pixels)."""
    try:
        recorded = read_run_state(args.ckpt)
    except (FileNotFoundError, NotADirectoryError) as e:
        ap.error(f"{args.command}: --ckpt {args.ckpt}: {e}")
    scene, _ = load_scene(ap, args, args.split, recorded, pixels=False)
    return scene


def _camera_source(ap: argparse.ArgumentParser, args, capture_errors=(FileNotFoundError,)):
    """Where --data [--split] [--data-format] / --poses / --scale-factor take a command's cameras from (the caller has seen to it
    that at most one of --data and --poses is given) -> (the capture's scene or None, what render.load_poses reads of the file or
    None): one of the two, or neither without both flags.  A Blender-format file carries no size: width and height are then the
    first image's, where there is one.  Host work only (JSON and image headers).  capture_errors: what reading a capture may raise
    that becomes an argparse error of the command."""
    from . import render

    if args.data is None:
        return None, None if args.poses is None else render.load_poses(args.poses, _scale_factor(args))
    from .data import detect_data_format

    try:
        if detect_data_format(args.data, args.data_format) == "nerfstudio":
            return _capture_cameras(ap, args), None
    except capture_errors as e:
        ap.error(f"{args.command}: {e}")
    src = render.load_poses(os.path.join(args.data, f"transforms_{args.split}.json"), _scale_factor(args))
    if src["width"] is None or src["height"] is None:
        rel = src["file_paths"][0] or ""
        path = os.path.join(args.data, (rel[2:] if rel.startswith("./") else rel) + ".png")
        if os.path.isfile(path):
            from PIL import Image

            with Image.open(path) as img:
                src["width"], src["height"] = (int(v) for v in img.size)
    return None, src


TSDF_ONLY_FLAGS = ("data", "poses", "max_views", "trunc", "min_weight", "ray_chunk")
TEXTURE_ONLY_FLAGS = ("texels", "min_footprint")


def resolve_texture_args(ap: argparse.ArgumentParser, args) -> None:
    """The texture flags of an `export-mesh` command line: --texels and --min-footprint need --texture; with it --out must end in
    .obj, --texels be at least 4 and --min-footprint lie above 0 and not above the largest spacing of the grid --bounds and
    --resolution make.  Host work only; what cannot work is an argparse error that names the option."""
    from . import mesh, texture

    if not args.texture:
        _flags_need(ap, args, TEXTURE_ONLY_FLAGS, "--texture")
        return
    if not args.out.lower().endswith(".obj"):
        ap.error(f"export-mesh: --texture writes an OBJ with its MTL and PNG maps: --out {args.out} must end in .obj")
    if args.texels is not None and not 4 <= args.texels <= texture.MAX_SIZE:
        ap.error(f"export-mesh: --texels {args.texels}: need a value from 4 to {texture.MAX_SIZE}")
    if args.min_footprint is not None:
        try:
            spacing = mesh.grid_frame(mesh.DEFAULT_BOUNDS if args.bounds is None else args.bounds, args.resolution)[2]
        except ValueError:
            return  # a grid that cannot be: the export says so
        try:
            texture.footprint_bounds(spacing, args.min_footprint)
        except ValueError as e:
            ap.error(f"export-mesh: --min-footprint {args.min_footprint}: {e}")


def resolve_decimate_args(ap: argparse.ArgumentParser, args) -> dict:
    """The decimation flags of an `export-mesh` command line -> the keyword arguments export_mesh takes for them ({} without the
    flags): --decimate-cells and --target-faces exclude each other and take values of at least 1; --target-faces searches up to the
    grid's intervals per axis, so it needs a --resolution of at least 3.  Host work only; what cannot work is an argparse error."""
    cells, faces = args.decimate_cells, args.target_faces
    if cells is not None and faces is not None:
        ap.error("export-mesh: --decimate-cells and --target-faces exclude each other")
    if cells is not None and cells < 1:
        ap.error(f"export-mesh: --decimate-cells {cells}: need a value of at least 1")
    if faces is not None and faces < 1:
        ap.error(f"export-mesh: --target-faces {faces}: need a value of at least 1")
    if faces is not None and args.resolution < 3:
        ap.error(f"export-mesh: --target-faces searches from 2 cells per axis up to the grid's intervals: --resolution {args.resolution} has fewer")
    return {k: v for k, v in (("decimate_cells", cells), ("target_faces", faces)) if v is not None}


def resolve_export_cameras(ap: argparse.ArgumentParser, args) -> Optional[dict]:
    """The cameras of an `export-mesh` command line: None for --method density (the tsdf flags are an error then), else {"c2w"
    [F,3,4], "width", "height", "fx", "fy", "cx", "cy"} after --max-views and --downscale.  Host work only (JSON and one image
    header).  What the command line leaves open and no file settles is an argparse error that names the option."""
    if args.method != "tsdf":
        _flags_need(ap, args, TSDF_ONLY_FLAGS, "--method tsdf", more=["--downscale"] if args.downscale != 1 else [])
        return None
    if args.iso is not None:
        ap.error("export-mesh: --iso is the density route's level; --method tsdf has none")
    cameras = export_cameras_from_args(ap, args, "export-mesh", "--method tsdf needs")
    if args.trunc is not None and not (math.isfinite(args.trunc) and args.trunc > 0.0):
        ap.error(f"export-mesh: --trunc {args.trunc}: need a finite value above 0")
    if args.min_weight is not None and not math.isfinite(args.min_weight):
        ap.error(f"export-mesh: --min-weight {args.min_weight}: need a finite value")
    if args.ray_chunk is not None and args.ray_chunk < 1:
        ap.error("export-mesh: --ray-chunk must be >= 1")
    return cameras


def export_cameras_from_args(ap: argparse.ArgumentParser, args, command: str, needs: str) -> dict:
    """The cameras --data [--split] / --poses [--scale-factor] [--max-views] [--downscale] name, for the export commands: {"c2w"
    [F,3,4], "width", "height", "fx", "fy", "cx", "cy"}.  Errors are argparse errors of `command`; `needs` words the one about
    missing cameras."""
    from . import render

    if (args.poses is None) == (args.data is None):
        ap.error(f"{command}: {needs} cameras: give --data DIR or --poses FILE.json (one of them)")
    capture, src = _camera_source(ap, args, capture_errors=(FileNotFoundError, ValueError))
    if capture is not None:
        from .data import shared_pinhole

        try:
            pinhole = shared_pinhole(capture, command)  # one pinhole for all views is what the export kernels project through
        except ValueError as e:
            ap.error(f"{command}: {e}")
        return _views_at_scale(ap, args, capture.c2w, capture.width, capture.height, *pinhole)
    for name in ("width", "height", "camera_angle_x"):
        if src[name] is None:
            ap.error(f"{command}: the cameras' {name} is unknown: the file needs camera_angle_x and w / h (or, with --data, a first image)")
    return _views_at_scale(ap, args, src["c2w"], src["width"], src["height"], *render.pinhole(src["width"], src["height"], src["camera_angle_x"]))


def _views_at_scale(ap: argparse.ArgumentParser, args, c2w, width, height, fx, fy, cx, cy) -> dict:
    """--max-views N evenly spaced ones of the views, the first one among them, at 1/--downscale of their size with the intrinsics
    scaled alike."""
    if args.downscale < 1 or (args.max_views is not None and args.max_views < 1):
        ap.error(f"{args.command}: --downscale and --max-views must be >= 1")
    if args.max_views is not None and args.max_views < len(c2w):
        c2w = c2w[(np.arange(args.max_views, dtype=np.int64) * len(c2w)) // args.max_views]
    w, h = max(1, width // args.downscale), max(1, height // args.downscale)
    sx, sy = w / width, h / height
    return {"c2w": np.ascontiguousarray(c2w), "width": int(w), "height": int(h), "fx": fx * sx, "fy": fy * sy, "cx": cx * sx, "cy": cy * sy}


def resolve_pointcloud_args(ap: argparse.ArgumentParser, args) -> dict:
    """The settings of an `export-pointcloud` command line: {"cameras" (as resolve_export_cameras returns them), "resolution",
    "bounds", "min_accumulation", "edge" (math.inf with --no-edge), "thin", "ray_chunk", "chunk"}.  What the command line alone
    settles is checked before any file is opened; every error is an argparse error that names the option."""
    from . import mesh

    if args.resolution < 1 or args.resolution ** 3 > 2 ** 27:
        ap.error(f"export-pointcloud: --resolution {args.resolution}: need 1 <= N <= 512")
    if not (math.isfinite(args.edge) and args.edge >= 0.0):
        ap.error(f"export-pointcloud: --edge {args.edge}: need a finite value >= 0 (--no-edge switches the test off)")
    if math.isnan(args.min_accumulation):
        ap.error(f"export-pointcloud: --min-accumulation {args.min_accumulation}: need a number")
    b = args.bounds
    _check_box(ap, args, "--bounds", b)
    if args.ray_chunk is not None and args.ray_chunk < 1:
        ap.error("export-pointcloud: --ray-chunk must be >= 1")
    if args.chunk is not None and args.chunk < 1:
        ap.error("export-pointcloud: --chunk must be >= 1")
    cameras = export_cameras_from_args(ap, args, "export-pointcloud", "needs")
    return {"cameras": cameras, "resolution": int(args.resolution), "bounds": mesh.DEFAULT_BOUNDS if b is None else tuple(float(x) for x in b),
            "min_accumulation": float(args.min_accumulation), "edge": math.inf if args.no_edge else float(args.edge),
            "thin": not args.no_thin, "ray_chunk": mesh.DEFAULT_RAY_CHUNK if args.ray_chunk is None else args.ray_chunk,
            "chunk": mesh.DEFAULT_CHUNK if args.chunk is None else args.chunk}


# ------------------------------------------------------------------------------------------------ train
def _resolve_run_settings(given: dict, recorded: Optional[dict]):
    """Each entry of `given` (names of checkpoint.RUN_SETTINGS, any subset): the caller's value if given, else the checkpoint's, else the
    table's fresh-run default (deterministic: None = the model's own default; the two guard settings and the coefficients of the opt-in
    loss terms: None = off; multiscale: 1, which a checkpoint does not record).
    -> (settings, one line per given value that departs from the checkpoint's)."""
    out, notes = {}, []
    for k, v in given.items():
        rec = None if recorded is None else recorded.get(k)
        if v is None:
            v = rec if rec is not None else RUN_SETTINGS[k].default
        elif rec is not None and v != rec:
            notes.append(f"train: {k} {v!r} given, the checkpoint's run had {rec!r}: using {v!r}; the continuation is not bit-exact")
        out[k] = v
    return out, notes


def _loss_key(name: str) -> str:
    """A coefficient's name in the model's config.loss_coefficients: the fine level's says so there."""
    return name + "_fine" if name in COEFFICIENTS and not name.endswith("_coarse") else name


def _settings_text(settings: dict) -> str:
    """The settings of a run as the line that starts it shows them: the ones its checkpoints record (recorded_settings), a float that
    is a setting of the optimiser or of a loss term in %g, everything else as it prints."""
    return "".join(f" {_loss_key(k)} {v:g}" if isinstance(v, float) and k not in RAY_KEYS else f" {_loss_key(k)} {v}"
                   for k, v in recorded_settings(settings).items())


def _guard_log(stats: dict, skips_logged: int) -> str:
    """The guard's part of a log line from FusedRAdam.guard_stats(); names the non-finite parameters of the last skipped step when
    steps were skipped since the line that reported `skips_logged` of them.  The optimiser's step_count of a step is its
    iteration number + 1."""
    text = f"  gnorm {stats['last_norm']:.4e} clip {stats['last_coef']:.4g} skipped {stats['skipped_total']}"
    if stats["skipped_total"] > skips_logged:
        bad = ", ".join(str(k) for k in stats["nonfinite_at_last_skip"])
        text += f" (step {stats['last_skipped_step'] - 1}: non-finite gradients in {bad})"
    return text


def train(scene, out_dir: str, steps: int = 100000, rays: Optional[int] = None, mma: Optional[str] = None, save_every: int = 1000,
          log_every: int = 100, seed: Optional[int] = None, device="cuda:0", model_config=None,
          log: Optional[Callable[[str], None]] = print, deterministic: Optional[bool] = None, resume: Optional[str] = None,
          on_step: Optional[Callable[[int, torch.Tensor], None]] = None, max_grad_norm: Optional[float] = None,
          skip_nonfinite: Optional[bool] = None, multiscale: Optional[int] = None, distortion_loss: Optional[float] = None,
          distortion_loss_coarse: Optional[float] = None, near: Optional[float] = None, far: Optional[float] = None,
          primary_spacing: Optional[str] = None, primary_tan: Optional[float] = None, data_settings: Optional[dict] = None,
          depth_loss: Optional[float] = None, depth_loss_coarse: Optional[float] = None, depth_sigma: Optional[float] = None,
          depth_euclidean: Optional[bool] = None) -> str:
    """Train on `scene` (a data.BlenderScene) up to iteration `steps` (the total, nerfstudio's max_num_iterations); returns the path
    of the last checkpoint.  Checkpoints at every step > 0 divisible by save_every and after the last step (nerfstudio's trainer
    does the same).  The loss is read back only every log_every steps: the iterations in between never wait for the GPU.
    rays / mma / seed: None = 1024 / "f32" / 0 (a resumed run: the checkpoint's).  deterministic: Model.set_deterministic (None: the
    checkpoint's when resuming, else the model's default, i.e. the environment's RSN_DETERMINISTIC); the line that starts the run
    records all four.  on_step(step, loss) is called after every step with the 0-d device tensor of train_step, which nothing here
    reads back for it.

    max_grad_norm / skip_nonfinite: FusedRAdam's guard (None: the checkpoint's when resuming, else off).  With either set, the
    log_every lines -- where the loss is read back anyway -- also read the optimiser's guard_stats(): the last step's gradient
    norm and clip factor and the number of steps skipped so far; the first such line after a skip names the parameters whose
    gradients were not finite on the last skipped step.  The steps in between read nothing.

    multiscale: the number of pyramid levels the rays are drawn from (RayDataManager's levels; None: the checkpoint's when resuming,
    else 1).  A batch stays a pure function of (seed, rank, step) and the pyramid one of the images, so the paragraph on the restored
    state below holds for a multi-scale run as it stands.

    distortion_loss / distortion_loss_coarse: the coefficient of the distortion loss (mip-NeRF 360 eq. 15) of the fine / the coarse
    level's weights (None: the checkpoint's when resuming, else off; 0 is off too).  A set coefficient goes into the model's
    config.loss_coefficients as "distortion_loss_fine" / "distortion_loss_coarse" (train_graph.DIST_COEF_KEYS), which switches the
    level's two launches on; mip-NeRF 360 uses 0.01, nerfacto 0.002, neither measured on this method.  The term reads no state beyond
    the step's own weights and bins, so the paragraph on the restored state below holds with it as it stands.

    depth_loss / depth_loss_coarse: the coefficient of the DS-NeRF depth term (include/rsn.h: rsn_depth_loss_forward) of the fine / the
    coarse level against the scene's depth maps (None: the checkpoint's when resuming, else off; 0 is off too); depth_sigma: its
    standard deviation in scene units (None: the checkpoint's, else the model's 0.1); depth_euclidean: the maps hold distances along
    the ray, not z-depths.  A set coefficient goes into config.loss_coefficients as "depth_loss_fine" / "depth_loss_coarse"
    (train_graph.DEPTH_COEF_KEYS) and needs scene.depths (ValueError otherwise); with both off the scene's depth maps are not
    uploaded and the step makes the launches it made before.  No scene has been measured: the values are starting points.  The
    targets are a pure function of the batch's pixels, so the paragraph on the restored state below holds with the term as it stands.

    near / far: the collider planes of the primary rays; primary_spacing / primary_tan: their coarse sampler, "uniform" or "reciprocal"
    with s(t) = t / (1/tan + t) (checkpoint.set_primary_sampler).  None: the checkpoint's when resuming; else, for a scene with a
    camera table (a capture), CAPTURE_RAY_DEFAULTS -- 0.05, 256, reciprocal, 1: starting points, not measured on a scene -- and for
    every other scene the model config's own (2, 6, uniform), with nothing recorded.  What is set is recorded in the checkpoint, and
    every tool that opens it casts its rays the same way.  data_settings: how the scene was read (load_scene); recorded as "data"
    together with the transform and scale the scene carries, which also go to out_dir/dataparser_transforms.json (nerfstudio's file).
    None of this is state a step leaves behind: the paragraph on the restored state below holds as it stands.

    resume: a step-*.ckpt or a run directory (its latest).  A checkpoint of step k continues at k + 1 with the same checkpoint names
    and save_every rule; k >= steps - 1 is a ValueError.  Model (strict, as load_checkpoint) and FusedRAdam state come from the file.
    From a checkpoint with `rsn_run` (every checkpoint this function writes) also both torch generators and, where not given here,
    rays / mma / seed / deterministic; a given value that differs is logged and used.  Without `rsn_run` the run continues with the
    arguments given and a fresh jitter stream, and says once that this is not bit-exact.

    Why the restored state is all of it (default settings: reflect_capacity None, weight_grad_groups 1, no ray_chunk).  A step reads:
    its batch, a pure function of (seed, rank, step) (RayDataManager.next_train); the loss coefficients and the learning rate,
    functions of the step and of FusedRAdam.step_count; the parameters and the moments; and the samplers' jitter from the device's
    torch generator (train_graph: torch.rand).  Everything else a step leaves behind is written before it is read in the next one:
    model._last_n_masked_dev / _step_n_masked_dev are this step's reflected-ray count, for diagnostics; the Field's packed weights
    are rebuilt whenever a parameter's version moved; the ordered reduction's workspace is never read before it is written
    (test_deterministic_gpu).  One value does travel between steps, only under the opt-in reflect_capacity = "auto": the reflected
    count that sizes the next step's reflect buffers.  It is not saved.  A resumed run starts with full-size buffers, which is
    the exact computation; it can differ from the uninterrupted run only on a step which that run truncated (and warned about)."""
    given = {k: v for k, v in locals().items() if k in RUN_SETTINGS}  # the arguments that are run settings, in the signature's order
    assert len(given) == len(RUN_SETTINGS)  # the signature spells out the table's names
    from .data import RayDataManager, pyramid_layout
    from .parallel import train_step
    from .train_ops import FusedRAdam

    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    first, model, ckpt, recorded = 0, None, None, None
    if resume is not None:  # host work only up to the ValueError: a run with nothing left to do never touches the device
        resume = resolve_checkpoint(resume)
        ckpt = torch.load(resume, map_location="cpu", weights_only=False)
        first = int(ckpt["step"]) + 1
        if first >= steps:
            raise ValueError(f"{resume} is at step {first - 1} and steps is {steps}: the run ends with step {steps - 1}, nothing is "
                             "left to train (steps is the total, not the number of further steps)")
        recorded = ckpt.get(RUN_STATE_KEY)
        if recorded is not None and recorded.get("version") != RUN_STATE_VERSION:
            raise ValueError(f"{resume}: {RUN_STATE_KEY} version {recorded.get('version')!r}, this trainer reads {RUN_STATE_VERSION}")
    cfg, notes = _resolve_run_settings(given, recorded)
    rays_cast = {k: cfg[k] for k in RAY_KEYS}
    if getattr(scene, "cameras", None) is not None:  # a capture: its own starting points where nothing else says
        rays_cast = {k: CAPTURE_RAY_DEFAULTS[k] if v is None else v for k, v in rays_cast.items()}
    if rays_cast["primary_spacing"] != "reciprocal":
        if given["primary_tan"] is not None:
            raise ValueError(f"primary_tan = {primary_tan} needs primary_spacing = 'reciprocal'")
        rays_cast["primary_tan"] = None
    if resume is not None:
        model, _ = _load_pipeline(resume, model_config, rays=rays_cast, ckpt=ckpt)
    rays, mma, seed, multiscale = cfg["rays"], cfg["mma"], cfg["seed"], int(cfg["multiscale"])
    for k in COEFFICIENTS:
        if cfg[k] is not None and not math.isfinite(float(cfg[k])):
            raise ValueError(f"{_loss_key(k)} must be finite, got {cfg[k]!r}")
    # the coefficients that switch a term on, under their names in the model's config.loss_coefficients (train_graph.DIST_COEF_KEYS, DEPTH_COEF_KEYS)
    terms_on = {_loss_key(k): float(cfg[k]) for k in COEFFICIENTS if cfg[k] is not None and float(cfg[k]) != 0.0}
    depth_on = [_loss_key(k) for k in COEFFICIENTS if _loss_key(k) in terms_on and RUN_SETTINGS[k].term == "depth"]
    if cfg["depth_sigma"] is not None and not (math.isfinite(float(cfg["depth_sigma"])) and float(cfg["depth_sigma"]) > 0.0):
        raise ValueError(f"depth_sigma must be a positive finite number, got {cfg['depth_sigma']!r}")
    if depth_on and getattr(scene, "depths", None) is None:
        raise ValueError(f"{' / '.join(depth_on)} set, but the scene has no depth maps (scene.depths is None): load it with "
                         "load_nerfstudio_split(..., depths=True) or build it with BlenderScene.from_arrays(..., depths=...)")
    if mma not in MMA_CHOICES:
        raise ValueError(f"mma must be one of {MMA_CHOICES}, got {mma!r}")
    pyramid_layout(scene.num_images, scene.height, scene.width, multiscale)  # a size the levels do not divide ends here, on the host
    dev = torch.device(device)
    if model is None:
        from .reflect_sampling_nerf_model import ReflectSamplingNeRFModelConfig

        planes = config_with_planes(model_config if model_config is not None else ReflectSamplingNeRFModelConfig(), rays_cast["near"],
                                    rays_cast["far"])
        model = make_model(planes, seed)
        set_primary_sampler(model, rays_cast["primary_spacing"], rays_cast["primary_tan"])
    model = model.to(dev).train()
    model.field.set_mma_mode(mma)
    if cfg["deterministic"] is not None:
        model.set_deterministic(cfg["deterministic"])
    if terms_on:  # (off: the dictionary stays as it is, without the keys.)  A copy: a model_config the caller shares between runs stays as it was
        model.config.loss_coefficients = dict(model.config.loss_coefficients, **terms_on)
    if depth_on:
        if cfg["depth_sigma"] is not None:
            model.depth_sigma = float(cfg["depth_sigma"])
    elif getattr(scene, "depths", None) is not None:  # the term is off: no upload, no gather launch, the batches as they always were
        import dataclasses

        scene = dataclasses.replace(scene, depths=None)
    dm = RayDataManager(scene, dev, num_rays_per_batch=rays, seed=seed, levels=multiscale, depth_euclidean=bool(cfg["depth_euclidean"]))
    params = model.get_param_groups()["fields"]
    name_of = {id(p): n for n, p in model.named_parameters()}
    optimizer = FusedRAdam(params, lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000,  # config.py:50-53
                           max_grad_norm=cfg["max_grad_norm"], skip_nonfinite=bool(cfg["skip_nonfinite"]), names=[name_of[id(p)] for p in params])
    run_settings = {**cfg, **rays_cast, "deterministic": model.deterministic}  # what the run goes by: what its checkpoints record
    settings = f"steps {steps}" + _settings_text(dict(run_settings, depth_sigma=model.depth_sigma))
    data_record = None
    if data_settings is not None:
        data_record = dict(data_settings)
        if getattr(scene, "dataparser_transform", None) is not None:
            from .data import write_dataparser_transforms

            data_record.update(transform=np.asarray(scene.dataparser_transform, dtype=np.float64).tolist(), scale=float(scene.dataparser_scale))
            write_dataparser_transforms(os.path.join(out_dir, "dataparser_transforms.json"), scene.dataparser_transform, scene.dataparser_scale)
    if resume is None:
        if log is not None:
            log(f"train: {settings}")
    else:
        optimizer.load_state_dict(ckpt["optimizers"]["fields"])
        if log is not None:
            log(f"train: resumed from {resume} at step {first - 1}: {settings}")
            for note in notes:
                log(note)
        if recorded is not None:
            torch.set_rng_state(recorded["cpu_rng_state"])
            if dev.type == "cuda" and recorded.get("cuda_rng_state") is not None:
                torch.cuda.set_rng_state(recorded["cuda_rng_state"], dev)
        elif log is not None:
            log(f"train: {resume} has no {RUN_STATE_KEY} entry (not written by this trainer): the sampling jitter starts a fresh "
                "stream, the continuation is not bit-exact")
        ckpt = None  # the host copy of the checkpoint is not needed past this point
    last = None
    skips_logged = 0
    t0 = time.time()
    for step in range(first, steps):
        ray_bundle, batch = dm.next_train(step)
        loss = train_step(model, ray_bundle, batch, optimizer, None, step)
        if on_step is not None:
            on_step(step, loss)
        if log is not None and log_every and (step % log_every == 0 or step == steps - 1):
            line = f"step {step:7d}  loss {float(loss):.6f}  lr {optimizer.current_lr():.3e}  {time.time() - t0:8.1f} s"
            if optimizer.guarded:
                stats = optimizer.guard_stats()  # one more read where the loss is read anyway
                line += _guard_log(stats, skips_logged)
                skips_logged = stats["skipped_total"]
            log(line)
        if (save_every and step > 0 and step % save_every == 0) or step == steps - 1:
            last = save_checkpoint(checkpoint_path(out_dir, step), model, optimizer, step,
                                   make_run_state(device=dev, data=data_record, **run_settings))
            if log is not None:
                log(f"saved {last}")
    return last


# ------------------------------------------------------------------------------------------------ eval
def _white(image: torch.Tensor) -> torch.Tensor:
    return image[..., :3] * image[..., 3:] + (1.0 - image[..., 3:]) if image.shape[-1] == 4 else image


MULTISCALE_NOTE = ("every view is scored at every scale 1/s, s = 1, 2, 4, ..., against the box average of the white-blended ground truth; "
                   "KEY_x<s> / KEY_x<s>_std are the mean and the unbiased standard deviation over the views at scale 1/s; the plain KEY "
                   "is the mean of the per-scale means and KEY_std the unbiased standard deviation of those means")
SSIM_WINDOW = 11  # include/rsn.h rsn_ssim
GEOMETRY_KEYS = ("normal_mae", "alpha_mae", "normal_weight")  # per_image, level 0
GEOMETRY_NOTE = ("normal_mae is the alpha-weighted mean angle in degrees between the composited predicted normal of the fine level, "
                 "sum_s w_s n_s (unnormalised: the angle does not depend on its length), and the ground-truth normal map, over the pixels "
                 "with alpha above 0 and a normal other than the background's (bytes 127 / 128); alpha_mae is the mean of |accumulation_fine "
                 "- alpha| over all pixels; both are scored on the full-resolution render only (with multiscale: level 0, no _x<s> variants, "
                 "not folded into a per-scale mean), results hold their mean and unbiased standard deviation over the views, views without "
                 "a pixel to score (normal_mae NaN) left out of normal_mae and counted out of normal_mae_views; the analytic (density-"
                 "gradient) normals are not scored: eval mode does not form them")
DEPTH_KEYS = ("depth_mae", "depth_rmse", "depth_valid")  # per_image, level 0
DEPTH_NOTE = ("depth_mae / depth_rmse are the mean absolute and the root mean square difference, in scene units, between depth_fine (the "
              "fine level's expected distance along the ray) and the distance along the ray that the view's depth map gives the pixel "
              "(a z-depth times the length of the pixel's un-normalised camera-space direction, unless the maps are euclidean), over the "
              "pixels with a measurement (depth > 0) and, where the split has masks, a live mask byte; depth_valid is their share of the "
              "view; scored on the full-resolution render only; results hold the mean and the unbiased standard deviation over the views "
              "with a scored pixel")
NORMAL_ERROR_DISPLAY_DEG = 45.0  # the error tile of NNNN_normals.png saturates here: a display range, not a measurement


def check_normals_request(scene, normals_space: str) -> None:
    """ValueError for an `evaluate(normals=True)` that cannot work; host checks only."""
    if normals_space not in NORMALS_SPACES:
        raise ValueError(f"normals_space = {normals_space!r}: choose from {', '.join(NORMALS_SPACES)}")
    if scene.normals is None:
        raise ValueError("normals=True needs a scene with ground-truth normal maps (scene.normals is None): load it with "
                         "load_blender_split(..., normals=True) or build it with BlenderScene.from_arrays(..., normals=...)")


def _save_normals_panel(path: str, outputs, gt_normals: torch.Tensor, gt_rgba: torch.Tensor, error_map: torch.Tensor) -> None:
    """predicted normals | ground-truth normals (the file's own frame) | error map, turbo over 0 .. 45 degrees: three rsn_visualize tiles."""
    from PIL import Image

    from . import render
    from ._abi import RSN_VIS_LUT, RSN_VIS_UNIT

    H, W = int(error_map.shape[0]), int(error_map.shape[1])
    panel = torch.empty(H, 3 * W, 3, dtype=torch.uint8, device=error_map.device)
    render.visualize(render.ray_normals(outputs).contiguous(), RSN_VIS_UNIT, panel, 0, alpha=outputs["accumulation_fine"].contiguous())
    gt = ((gt_normals.to(torch.float32) * 2.0 - 255.0) / 255.0).contiguous()
    render.visualize(gt, RSN_VIS_UNIT, panel, W, alpha=(gt_rgba[..., 3].to(torch.float32) / 255.0).contiguous())
    render.visualize(error_map.contiguous(), RSN_VIS_LUT, panel, 2 * W, lo=0.0, hi=NORMAL_ERROR_DISPLAY_DEG, lut=render.turbo_lut(error_map.device))
    Image.fromarray(panel.cpu().numpy()).save(path)


def eval_level_sizes(scene, multiscale: int):
    """((H, W) of level 0 .. multiscale-1) of the scene's views; ValueError for a level count outside 1 .. 5, a size 2^(multiscale-1)
    does not divide, and a smallest level below the 11 x 11 pixels SSIM needs.  Host arithmetic only."""
    from .data import pyramid_layout

    sizes, _ = pyramid_layout(scene.num_images, scene.height, scene.width, multiscale)
    if multiscale > 1 and min(sizes[-1]) < SSIM_WINDOW:
        raise ValueError(f"multiscale {multiscale}: the views of level {multiscale - 1} are {sizes[-1][1]} x {sizes[-1][0]} pixels, "
                         f"SSIM needs at least {SSIM_WINDOW} x {SSIM_WINDOW}")
    return sizes


def evaluate(scene, ckpt: str, max_images: Optional[int] = None, save_images: Optional[str] = None, device="cuda:0",
             model_config=None, occupancy: Optional[dict] = None, multiscale: int = 1, normals: bool = False,
             normals_space: str = "world", depth: bool = False, depth_euclidean: bool = False) -> dict:
    """Score the checkpoint (a file, or the latest of a run directory) on every view of `scene` (a data.BlenderScene); -> ns-eval-
    shaped dict.  occupancy: None, or the settings of resolve_occupancy_args: the views are rendered with empty-space skipping and
    the dict gains an "occupancy" entry.  A scene with a camera table (a capture) is rendered through its own cameras; the occupancy
    box alone is laid out from the first camera's pinhole part.

    multiscale = L > 1: every view is rendered and scored at the L levels of RayDataManager's pyramid.  per_image then holds one entry
    per (view, level) with a "level" key, view after view; results gains k_x1, k_x2, k_x4, ... (+ _std) for every metric k, the mean
    over the views at that level; the plain k is the mean of the per-level means, and a "multiscale" entry says so.  The occupancy grid
    is built once, from the full-resolution cameras (whose frusta are those of every level), and culls the rays of every level.
    ValueError, before the checkpoint is read, when the smallest level is below the 11 x 11 pixels SSIM needs.

    normals=True: the geometry metrics of metrics.normal_error against scene.normals (ValueError, before the checkpoint is read, when
    the scene has none).  Every level-0 entry of per_image gains normal_mae, alpha_mae and normal_weight; results gains normal_mae,
    normal_mae_std, alpha_mae, alpha_mae_std and normal_mae_views, and the dict a "geometry" entry (GEOMETRY_NOTE).  normals_space
    "camera": the maps are in each view's camera frame.  With save_images, NNNN_normals.png: prediction | ground truth | error.
    normals=False is the evaluation without any of it: the same launches, keys and bytes.

    A scene with masks (a capture's): psnr / ssim stay those of the whole image, as nerfstudio reports them; every level-0 entry of
    per_image gains psnr_masked, the fine PSNR over the live pixels alone (nan for a view without one), and results psnr_masked and
    psnr_masked_std over the views that have one.  It is formed on the device from the tensors of the view and read once, after the
    last view.  Without masks nothing is added.

    depth=True: the depth metrics of metrics.depth_error (rsn_depth_error) against scene.depths (ValueError, before the checkpoint is
    read, when the scene has none): every view's depth_fine against the distance along the ray its depth map gives every pixel
    (RayDataManager.view_ray_depth; depth_euclidean: the maps hold such distances already, not z-depths), over the pixels with a
    measurement and, where the split has masks, a live mask byte.  Every level-0 entry of per_image gains depth_mae, depth_rmse (scene
    units) and depth_valid, the share of the view's pixels that were scored; results gains depth_mae, depth_rmse (+ _std, over the views
    with a scored pixel) and depth_valid (the mean share), and the dict a "depth" entry (DEPTH_NOTE).  The figures are formed on the
    device and read once, after the last view.  depth=False is the evaluation without any of it: the same launches, keys and bytes."""
    import dataclasses

    from . import metrics
    from .data import RayDataManager

    multiscale = int(multiscale)
    sizes = eval_level_sizes(scene, multiscale)
    if normals:
        check_normals_request(scene, normals_space)
    if depth and getattr(scene, "depths", None) is None:
        raise ValueError("depth=True needs a scene with depth maps (scene.depths is None): load it with "
                         "load_nerfstudio_split(..., depths=True) or build it with BlenderScene.from_arrays(..., depths=...)")
    if not depth and getattr(scene, "depths", None) is not None:
        scene = dataclasses.replace(scene, depths=None)  # nothing is uploaded
    dev = torch.device(device)
    ckpt, model, step = open_checkpoint(ckpt, model_config, dev)
    model.config.eval_num_rays_per_chunk = EVAL_CHUNK
    dm = RayDataManager(scene, dev, levels=multiscale, live_lists=False, depth_euclidean=depth_euclidean)
    masked, depth_scores = [], []  # (entry of per_image, device [K]) pairs: the live pixels' PSNR (K = 1) and DEPTH_KEYS' three figures
    n = scene.num_images if max_images is None else min(int(max_images), scene.num_images)
    if occupancy is not None:
        from .occupancy import attach_occupancy

        attach_occupancy(model, occupancy, scene.c2w[:n], scene.height, scene.width, scene.fx, scene.fy, scene.cx, scene.cy)
    if save_images:
        os.makedirs(save_images, exist_ok=True)
    per_image = []
    for i, level in ((i, level) for i in range(n) for level in range(multiscale)):
        torch.cuda.synchronize(dev)
        t0 = time.time()
        outputs = model.get_outputs_for_camera_ray_bundle(dm.camera_ray_bundle(i, level))
        gt = dm.image(i, level)
        m, images = model.get_image_metrics_and_images(outputs, {"image": gt})
        m = dict(m)
        m["fine_ssim"] = float(metrics.ssim(torch.clip(outputs["mid_reflect_fine"], 0.0, 1.0), _white(gt)))
        dt = time.time() - t0
        m["num_rays_per_sec"] = sizes[level][0] * sizes[level][1] / dt
        m["fps"] = 1.0 / dt
        if normals and level == 0:  # after the clock: the rates above are those of the evaluation without it
            composited = (outputs["weights_fine"] * outputs["pred_normals_fine"]).sum(dim=-2)
            geo = metrics.normal_error(composited, outputs["accumulation_fine"], dm.normal_image(i), dm.images[i],
                                       c2w=dm.c2w[i] if normals_space == "camera" else None, error_map=bool(save_images))
            m.update({k: float(geo[k]) for k in GEOMETRY_KEYS})
            if save_images:
                _save_normals_panel(os.path.join(save_images, f"{i:04d}_normals.png"), outputs, dm.normal_image(i), dm.images[i],
                                    geo["error_map"])
        per_image.append({"image": i, **({"level": level} if multiscale > 1 else {}), **m})
        if depth and level == 0:
            de = metrics.depth_error(outputs["depth_fine"], dm.view_ray_depth(i), dm.mask_image(i) if dm.masks is not None else None)
            depth_scores.append((per_image[-1], torch.stack([de[k] for k in DEPTH_KEYS])))
        if dm.masks is not None and level == 0:
            live = dm.mask_image(i).to(torch.float32).unsqueeze(-1)
            err = ((torch.clip(outputs["mid_reflect_fine"], 0.0, 1.0) - _white(gt)) ** 2 * live).sum() / (3.0 * live.sum())  # 0 / 0 = nan
            masked.append((per_image[-1], (10.0 * torch.log10(1.0 / err.clamp(min=1e-12))).reshape(1)))
        if save_images:
            from PIL import Image

            panel = (images["img"].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
            name = f"{i:04d}_img.png" if level == 0 else f"{i:04d}_x{1 << level}_img.png"
            Image.fromarray(panel).save(os.path.join(save_images, name))
    for scores, names in ((masked, ("psnr_masked",)), (depth_scores, DEPTH_KEYS)):
        if scores:
            for (entry, _), v in zip(scores, torch.stack([v for _, v in scores]).cpu().tolist()):  # the one read of these scores
                entry.update({k: float(x) for k, x in zip(names, v)})
    keys = [k for k in per_image[0] if k not in ("image", "level", "psnr_masked") + GEOMETRY_KEYS + DEPTH_KEYS] if per_image else []

    def mean_std(v):
        v = np.asarray(v, dtype=np.float64)
        if not len(v):  # no view had a value to count
            return float("nan"), float("nan")
        return float(v.mean()), float(v.std(ddof=1)) if len(v) > 1 else 0.0  # torch.std_mean (ns-eval): unbiased

    results = {}
    for k in keys:
        if multiscale == 1:
            results[k], results[k + "_std"] = mean_std([p[k] for p in per_image])
            continue
        per_level = [mean_std([p[k] for p in per_image if p["level"] == level]) for level in range(multiscale)]
        results[k], results[k + "_std"] = mean_std([m for m, _ in per_level])
        for level, (m, sd) in enumerate(per_level):
            results[f"{k}_x{1 << level}"], results[f"{k}_x{1 << level}_std"] = m, sd
    if masked:
        counted = [p["psnr_masked"] for p, _ in masked if not math.isnan(p["psnr_masked"])]
        results["psnr_masked"], results["psnr_masked_std"] = mean_std(counted)
    if normals:
        scored = [p for p in per_image if "normal_mae" in p]
        counted = [p["normal_mae"] for p in scored if not math.isnan(p["normal_mae"])]
        results["normal_mae"], results["normal_mae_std"] = mean_std(counted)
        results["normal_mae_views"] = len(counted)
        results["alpha_mae"], results["alpha_mae_std"] = mean_std([p["alpha_mae"] for p in scored])
    if depth:
        scored = [p for p, _ in depth_scores]
        for k in ("depth_mae", "depth_rmse"):
            counted = [p[k] for p in scored if not math.isnan(p[k])]
            results[k], results[k + "_std"] = mean_std(counted)
        results["depth_valid"] = float(np.mean([p["depth_valid"] for p in scored])) if scored else float("nan")
    res = {"experiment_name": os.path.basename(os.path.dirname(os.path.abspath(ckpt))), "method_name": METHOD_NAME,
           "checkpoint": ckpt, "step": step, "results": results, "not_computed": {"fine_lpips": LPIPS_NOTE},
           "per_image": per_image}
    if multiscale > 1:
        res["multiscale"] = {"levels": multiscale, "scales": [1 << level for level in range(multiscale)], "note": MULTISCALE_NOTE}
    if occupancy is not None:
        res["occupancy"] = model.occupancy.describe()
    if normals:
        res["geometry"] = {"normals_space": normals_space, "note": GEOMETRY_NOTE}
    if depth:
        res["depth"] = {"euclidean": bool(depth_euclidean), "note": DEPTH_NOTE}
    return res


# ------------------------------------------------------------------------------------------------ CLI
# Per command: `_check_*` holds what the command line alone (and host-side file headers) can rule out, and returns what it resolved
# on the way; `_run_*` is the command itself, on a machine with a GPU.
def _check_train(ap: argparse.ArgumentParser, args):
    for flag, v in (("--primary-tan", args.primary_tan), ("--max-grad-norm", args.max_grad_norm)):
        if v is not None and not v > 0.0:
            ap.error(f"train: {flag} {v}: need a value above 0")
    _check_multiscale(ap, args)


def _check_multiscale(ap: argparse.ArgumentParser, args) -> None:
    if not 1 <= args.multiscale <= 5:
        ap.error(f"{args.command}: --multiscale {args.multiscale}: need 1 to 5")


def _run_train(ap: argparse.ArgumentParser, args, given, _) -> None:
    resumed = read_run_state(args.resume) if args.resume is not None else None
    depth_coefficients = [k for k in COEFFICIENTS if RUN_SETTINGS[k].term == "depth"]
    depth_flags = ["--" + k.replace("_", "-") for k in depth_coefficients if getattr(args, k)]
    want_depth = bool(depth_flags) or any((resumed or {}).get(k) for k in depth_coefficients)
    if not want_depth:
        _flags_need(ap, args, ("depth_sigma", "depth_unit_scale", "depth_euclidean"), "--depth-loss or --depth-loss-coarse")
    if args.depth_sigma is not None and not args.depth_sigma > 0.0:
        ap.error(f"train: --depth-sigma {args.depth_sigma}: need a value above 0")
    scene, data_settings = load_scene(ap, args, "train", resumed, depths=want_depth)
    if want_depth and scene.depths is None:
        ap.error(f"train: {' '.join(depth_flags) or 'the resumed run'} needs depth maps, and no frame of {args.data} has a depth_file_path")
    print(f"{args.data}: {scene.num_images} train images {scene.width} x {scene.height}, focal {scene.fx:.3f}"
          + ("" if scene.cameras is None else f" (image 0; a capture with {len(np.unique(scene.cameras, axis=0))} distinct camera(s), "
                                              f"{int(np.any(scene.cameras[:, 4:] != 0.0, axis=1).sum())} image(s) with lens distortion)"))
    if args.multiscale > 1:  # a resumed run's own level count is checked by train()
        from .data import pyramid_layout

        try:
            pyramid_layout(scene.num_images, scene.height, scene.width, args.multiscale)
        except ValueError as e:
            ap.error(f"train: --multiscale {args.multiscale}: {e}")
    # every run setting as the user typed it, None where nothing was typed (`given`: the parse without the run defaults; a switch
    # that is off was not typed): a resumed run's checkpoint decides those
    typed = {k: None if getattr(given, k) is False else getattr(given, k) for k in RUN_SETTINGS}
    train(scene, args.out, steps=args.steps, save_every=args.save_every, log_every=args.log_every, resume=args.resume,
          data_settings=data_settings, **typed)


def _check_export_mesh(ap: argparse.ArgumentParser, args):
    resolve_texture_args(ap, args)
    decimate_args = resolve_decimate_args(ap, args)
    return decimate_args, resolve_export_cameras(ap, args)


def _run_export_mesh(ap: argparse.ArgumentParser, args, given, resolved) -> None:
    from . import mesh

    decimate_args, export_cameras = resolved
    common = dict(resolution=args.resolution, bounds=mesh.DEFAULT_BOUNDS if args.bounds is None else tuple(args.bounds),
                  mma=args.mma, chunk=mesh.DEFAULT_CHUNK if args.chunk is None else args.chunk)
    if args.texture:
        common.update(texture=True, texels=8 if args.texels is None else args.texels, min_footprint=args.min_footprint)
    common.update(decimate_args)
    if args.method == "tsdf":
        res = mesh.export_mesh(args.ckpt, args.out, method="tsdf", cameras=export_cameras, trunc=args.trunc,
                               min_weight=mesh.DEFAULT_MIN_WEIGHT if args.min_weight is None else args.min_weight,
                               ray_chunk=mesh.DEFAULT_RAY_CHUNK if args.ray_chunk is None else args.ray_chunk, **common)
        what = (f"of {res['views']} depth maps {res['image'][0]} x {res['image'][1]} fused at truncation {res['trunc']:g} "
                f"({res['triangles_extracted']} triangles before the filter)")
        stages = ("depth", "integrate", "count", "emit", "filter", "attributes", "write")
    else:
        res = mesh.export_mesh(args.ckpt, args.out, iso=mesh.DEFAULT_ISO if args.iso is None else args.iso, **common)
        what = f"at sigma = {res['iso']:g}"
        stages = ("grid", "count", "emit", "attributes", "write")
    sec = res["seconds"]
    if decimate_args:
        d = res["decimate"]
        stages = stages[:stages.index("attributes")] + ("decimate",) + stages[stages.index("attributes"):]
        what += (f", clustered from {d['triangles_in']} triangles with {' x '.join(str(n) for n in d['cells'])} cells "
                 f"({d['degenerate']} collapsed, {d['cancelled_pairs']} opposite pairs cancelled"
                 + (f", {len(d['probes'])} probes for at most {d['target_faces']}" + (": NOT reached" if d["over_budget"] else "")
                    if "probes" in d else "") + ")")
    if args.texture:
        stages = stages[:-1] + ("atlas", "bake", "write")
        what += (f", textured with {res['texture_size']} x {res['texture_size']} texels ({res['live_texels']} live, "
                 f"{res['texels']} per square side, footprint >= {res['min_footprint']:g})")
    print(f"{res['checkpoint']} (step {res['step']}): {res['vertices']} vertices, {res['triangles']} triangles {what} "
          f"on a {' x '.join(str(n) for n in res['resolution'])} grid; " +
          " ".join(f"{k} {sec[k]:.3f} s" for k in stages) + f" -> {res['out']}")


def _run_export_pointcloud(ap: argparse.ArgumentParser, args, given, cloud_args) -> None:
    from . import pointcloud

    res = pointcloud.export_pointcloud(args.ckpt, args.out, cloud_args.pop("cameras"), mma=args.mma, **cloud_args)
    sec = res["seconds"]
    print(f"{res['checkpoint']} (step {res['step']}): a grid of {' x '.join(str(n) for n in res['resolution'])} cells, "
          f"accumulation >= {res['min_accumulation']:g}, edge {res['edge']:g}, {'one point per cell' if res['thin'] else 'every candidate'}; " +
          " ".join(f"{k} {sec[k]:.3f} s" for k in ("depth", "mark", "select", "attributes", "write")))
    print(f"{res['points']} points from {res['views']} depth maps {res['image'][0]} x {res['image'][1]} "
          f"({res['candidates']} candidates) -> {res['out']}")


def _check_render(ap: argparse.ArgumentParser, args):
    cameras = resolve_render_args(ap, args)
    return cameras, resolve_occupancy_args(ap, args)


def _run_render(ap: argparse.ArgumentParser, args, given, resolved) -> None:
    from . import render

    cameras, occupancy = resolved
    res = render.render_checkpoint(args.ckpt, args.out, *render.camera_args(cameras), camera_table=cameras.get("camera_table"),
                                   channels=args.channels,
                                   depth_range=None if args.depth_range is None else tuple(args.depth_range), mma=args.mma,
                                   chunk=args.chunk, tiles=args.tiles, occupancy=occupancy)
    n, sec = len(res["frames"]), res["seconds"]
    print(f"{res['checkpoint']} (step {res['step']}): {n} frames {res['width']} x {res['height']} of {' '.join(res['channels'])}; "
          f"{sec / max(n, 1):.3f} s per frame, {n * res['width'] * res['height'] / max(sec, 1e-9):.0f} rays/s -> {res['out']}")


def _check_eval(ap: argparse.ArgumentParser, args):
    occupancy = resolve_occupancy_args(ap, args)
    if not args.depth:
        _flags_need(ap, args, ("depth_unit_scale", "depth_euclidean"), "--depth")
    if args.normals and args.depth:
        ap.error("eval: --normals scores a Blender-format scene and --depth a nerfstudio-format capture; give one of them")
    if not args.normals:
        _flags_need(ap, args, ("normals_suffix", "normals_space"), "--normals")
    _check_multiscale(ap, args)
    return occupancy


def _run_eval(ap: argparse.ArgumentParser, args, given, occupancy) -> None:
    try:
        recorded = read_run_state(args.ckpt)
    except (FileNotFoundError, NotADirectoryError) as e:
        ap.error(f"eval: --ckpt {args.ckpt}: {e}")
    if args.normals:
        scene, _ = load_scene(ap, args, args.split, recorded, normals=True,
                              normals_suffix=DEFAULT_NORMALS_SUFFIX if args.normals_suffix is None else args.normals_suffix)
    else:
        scene, _ = load_scene(ap, args, args.split, recorded, depths=args.depth)
    if args.depth and scene.depths is None:
        ap.error(f"eval: --depth needs depth maps, and no frame of the {args.split} split of {args.data} has a depth_file_path")
    try:
        eval_level_sizes(scene, args.multiscale)
    except ValueError as e:
        ap.error(f"eval: {e}")
    geometry = dict(normals=True, normals_space=args.normals_space or "world") if args.normals else {}
    if args.depth:
        euclid = args.depth_euclidean if args.depth_euclidean is not None else bool((recorded or {}).get("depth_euclidean"))
        geometry.update(depth=True, depth_euclidean=bool(euclid))
    res = evaluate(scene, args.ckpt, max_images=args.max_images, save_images=args.save_images, occupancy=occupancy,
                   multiscale=args.multiscale, **geometry)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=2)
    r = res["results"]
    for level in range(args.multiscale if args.multiscale > 1 else 0):
        print(f"  1/{1 << level}: " + " ".join(f"{k} {r[f'{k}_x{1 << level}']:.4f}" for k in ("psnr", "coarse_psnr", "fine_psnr", "fine_ssim")
                                        if f"{k}_x{1 << level}" in r and not math.isnan(r[f"{k}_x{1 << level}"])))
    print(" ".join(f"{k} {r[k]:.4f}" for k in ("psnr", "coarse_psnr", "fine_psnr", "fine_ssim") if k in r
                   and not math.isnan(r[k])) + f"  ({len(res['per_image'])} images) -> {args.out}")
    if args.normals:
        print(f"normal_mae {r['normal_mae']:.3f} deg over {r['normal_mae_views']} views, alpha_mae {r['alpha_mae']:.4f}")
    if args.depth:
        print(f"depth_mae {r['depth_mae']:.5f} depth_rmse {r['depth_rmse']:.5f} over {100.0 * r['depth_valid']:.1f} % of the pixels")


COMMANDS = {"train": (_check_train, _run_train), "eval": (_check_eval, _run_eval), "export-mesh": (_check_export_mesh, _run_export_mesh),
            "export-pointcloud": (resolve_pointcloud_args, _run_export_pointcloud), "render": (_check_render, _run_render)}


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    given = build_parser(run_defaults=False).parse_args(argv)  # None where the user typed nothing: a resumed run's checkpoint decides
    check, run = COMMANDS[args.command]
    resolved = check(ap, args)  # a command line that cannot work ends here
    if not torch.cuda.is_available():
        print("reflect_sampling_nerf_amd.trainer needs a GPU (the HIP kernels have no CPU path)", file=sys.stderr)
        return 2
    run(ap, args, given, resolved)
    return 0


if __name__ == "__main__":
    sys.exit(main())
