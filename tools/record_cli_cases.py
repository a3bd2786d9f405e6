"""Records what the command line and the run-settings plumbing of trainer.py / checkpoint.py compute on the host, into
tests/golden/cli_cases.json: what the five sub-commands parse to, what make_run_state records and _resolve_run_settings resolves,
how capture_load_args reads a capture, the text of the argparse errors that main() and the resolve_* functions end with, and the
cameras those functions resolve from small files written here.  No GPU is needed: every main() line recorded ends before main()
asks for one (asking is an AssertionError here).  tests/test_cli_cases_cpu.py compares the tree with the record; re-record only
with a change that is meant to move a flag, a default, a message or a checkpoint key.
  python tools/record_cli_cases.py [--out tests/golden/cli_cases.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
from unittest import mock

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import checkpoint, data, trainer  # noqa: E402

GROUPS = ("parses", "run_state", "capture_args", "main_errors", "resolved", "train_calls")
NOT_GIVEN = "<not given>"  # how the default of --scale-factor is written: 1.0 to arithmetic, and not a value the user typed
W, H = 8, 6


def plain(x):
    """x as JSON writes it: arrays as lists, floats as they are (repr round-trips), the not-given scale factor by name."""
    if isinstance(x, trainer._NotGiven):
        return NOT_GIVEN
    if isinstance(x, argparse.Namespace):
        return plain(vars(x))
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return plain(x.tolist())
    if isinstance(x, np.generic):
        return x.item()
    return x


def value_or_error(fn, *args):
    """What fn returns, or {"error": the text after "error: "} when it ends as argparse's error() does (usage and message on stderr,
    SystemExit)."""
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err):
            return plain(fn(*args))
    except SystemExit:
        return {"error": err.getvalue().split("error: ", 1)[1].strip()}


def error_of(fn, *args):
    value = value_or_error(fn, *args)
    assert isinstance(value, dict) and set(value) == {"error"}, f"{fn.__name__}{args}: no error"
    return value["error"]


# ------------------------------------------------------------------------------------------------ parses
CAPTURE_FLAGS = ["--data-format", "nerfstudio", "--orientation", "none", "--no-auto-scale", "--train-split-fraction", "0.5", "--eval-mode", "all",
                 "--downscale-factor", "2"]
OCCUPANCY_FLAGS = ["--skip-empty", "--skip-empty-samples", "--occupancy-resolution", "64", "--occupancy-sigma", "0.5", "--occupancy-dilate", "2",
                   "--occupancy-bounds", "-1", "-1", "-1", "1", "1", "1"]
PARSES = {
    "train": (["train", "--data", "d", "--out", "o"],
              ["--steps", "7", "--rays", "256", "--mma", "bf16", "--save-every", "3", "--log-every", "2", "--seed", "5", "--deterministic",
               "--scale-factor", "0.5", "--max-grad-norm", "1.5", "--skip-nonfinite", "--multiscale", "3", "--distortion-loss", "0.01",
               "--distortion-loss-coarse", "0.002", "--depth-loss", "0.1", "--depth-loss-coarse", "0.05", "--depth-sigma", "0.2",
               "--depth-unit-scale", "0.0005", "--depth-euclidean", "--center", "none", "--near", "0.25", "--far", "12", "--primary-spacing",
               "reciprocal", "--primary-tan", "2", "--resume", "r"] + CAPTURE_FLAGS),
    "eval": (["eval", "--data", "d", "--ckpt", "c"],
             ["--split", "val", "--max-images", "2", "--out", "m.json", "--save-images", "img", "--scale-factor", "0.5", "--center-poses", "none",
              "--multiscale", "2", "--normals", "--normals-suffix", "_n", "--normals-space", "camera", "--depth", "--depth-unit-scale", "0.002",
              "--depth-euclidean"] + CAPTURE_FLAGS + OCCUPANCY_FLAGS),
    "export-mesh": (["export-mesh", "--ckpt", "c", "--out", "m.ply"],
                    ["--resolution", "32", "--bounds", "-1", "-1", "-1", "1", "1", "1", "--iso", "5", "--mma", "bf16x6", "--chunk", "100", "--method",
                     "tsdf", "--data", "d", "--split", "val", "--poses", "p.json", "--scale-factor", "0.5", "--center-poses", "none", "--max-views",
                     "3", "--downscale", "2", "--trunc", "0.1", "--min-weight", "2", "--ray-chunk", "64", "--texture", "--texels", "16",
                     "--min-footprint", "0.01", "--decimate-cells", "8", "--target-faces", "100"] + CAPTURE_FLAGS),
    # --edge and --no-edge exclude each other in the parser: the full line has the former
    "export-pointcloud": (["export-pointcloud", "--ckpt", "c", "--out", "c.ply"],
                          ["--data", "d", "--split", "val", "--poses", "p.json", "--scale-factor", "0.5", "--center-poses", "none", "--max-views", "3",
                           "--downscale", "2", "--resolution", "64", "--bounds", "-1", "-1", "-1", "1", "1", "1", "--min-accumulation", "0.25",
                           "--edge", "0.1", "--no-thin", "--mma", "bf16", "--ray-chunk", "64", "--chunk", "100"] + CAPTURE_FLAGS),
    "render": (["render", "--ckpt", "c", "--out", "o"],
               ["--path", "poses", "--frames", "4", "--center", "0.1", "0.2", "0.3", "--radius", "3", "--elevation", "20", "--azimuth", "45", "--poses",
                "p.json", "--data", "d", "--split", "val", "--scale-factor", "0.5", "--center-poses", "none", "--interpolate", "2", "--width", "16",
                "--height", "12", "--fov-x", "50", "--channels", "rgb", "depth", "--depth-range", "1", "5", "--mma", "bf16", "--chunk", "512",
                "--tiles"] + CAPTURE_FLAGS + OCCUPANCY_FLAGS),
}


def parses():
    out = {}
    for command, (minimal, more) in PARSES.items():
        for which, argv in (("minimal", minimal), ("full", minimal + more)):
            for run_defaults in (True, False):
                out[f"{command} {which} run_defaults={run_defaults}"] = plain(trainer.build_parser(run_defaults=run_defaults).parse_args(argv))
    return out


# ------------------------------------------------------------------------------------------------ run state
DATA_RECORD = {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS, "transform": np.eye(4)[:3].tolist(), "scale": 0.25}
OPTIONAL = {"max_grad_norm": 2, "skip_nonfinite": True, "multiscale": 3, "distortion_loss": 0.01, "distortion_loss_coarse": 0.002, "near": 0.5,
            "far": 1.5, "primary_spacing": "reciprocal", "primary_tan": 2.0, "depth_loss": 0.1, "depth_loss_coarse": 0.05, "depth_sigma": 0.2,
            "depth_euclidean": True, "data": DATA_RECORD}
COEFFICIENTS = ("distortion_loss", "distortion_loss_coarse", "depth_loss", "depth_loss_coarse")
RUN_KEYS = ("rays", "mma", "seed", "deterministic") + tuple(k for k in OPTIONAL if k != "data")


def run_state(seed=0, rays=1024, mma="f32", deterministic=False, **settings):
    state = checkpoint.make_run_state(seed, rays, mma, deterministic, "cpu", **settings)
    assert isinstance(state.pop("cpu_rng_state"), torch.Tensor) and state.pop("cuda_rng_state") is None
    return plain(state)


def run_states():
    out = {"nothing set": run_state(), "every optional setting None": run_state(**dict.fromkeys(OPTIONAL)),
           "the four that are always recorded": run_state(7, 512, "bf16", True), "multiscale 1": run_state(multiscale=1),
           "skip_nonfinite False": run_state(skip_nonfinite=False), "depth_euclidean False with a coefficient": run_state(depth_loss=0.1, depth_euclidean=False),
           "depth_sigma and depth_euclidean without a coefficient": run_state(depth_sigma=0.2, depth_euclidean=True),
           "depth_sigma and depth_euclidean with the coarse coefficient": run_state(depth_loss_coarse=0.05, depth_sigma=0.2, depth_euclidean=True),
           "depth_sigma with both coefficients 0": run_state(depth_loss=0.0, depth_loss_coarse=0, depth_sigma=0.2),
           "all set": run_state(7, 512, "bf16", True, **OPTIONAL)}
    for k, v in OPTIONAL.items():
        out[f"{k} alone"] = run_state(**{k: v})
    for k in COEFFICIENTS:
        out[f"{k} 0"] = run_state(**{k: 0.0})
    try:
        run_state(depth=1)
    except KeyError:
        out["an unknown name"] = "KeyError"
    return out


def resolved_settings():
    recorded = checkpoint.make_run_state(7, 512, "bf16", True, "cpu", **OPTIONAL)
    typed = {"rays": 256, "mma": "bf16x6", "seed": 1, "deterministic": False, "max_grad_norm": 3.0, "skip_nonfinite": False, "multiscale": 2,
             "distortion_loss": 0.02, "distortion_loss_coarse": 0.004, "near": 0.25, "far": 3.0, "primary_spacing": "uniform", "primary_tan": 4.0,
             "depth_loss": 0.2, "depth_loss_coarse": 0.1, "depth_sigma": 0.4, "depth_euclidean": False}
    assert tuple(typed) == RUN_KEYS
    nothing = dict.fromkeys(RUN_KEYS)
    cases = {"fresh": (nothing, None), "fresh, typed": (typed, None), "resumed, nothing stated": (nothing, recorded),
             "resumed from a plain run": (nothing, checkpoint.make_run_state(0, 1024, "f32", False, "cpu")),
             "resumed, everything overridden": (typed, recorded), "resumed, the same values stated": ({k: recorded[k] for k in RUN_KEYS}, recorded),
             "a subset of the keys": ({"rays": None, "depth_sigma": 0.4}, recorded)}
    out = {}
    for name, (given, rec) in cases.items():
        settings, notes = trainer._resolve_run_settings(given, rec)
        out[name] = {"settings": plain(settings), "order": list(settings), "notes": notes}
    return out


# ------------------------------------------------------------------------------------------------ capture arguments
def capture_args():
    ap = trainer.build_parser()
    rec = {"data": {**DATA_RECORD, "orientation": "none", "train_split_fraction": 0.5, "downscale_factor": 4, "depth_unit_scale": 0.004}}
    cases = {"train": (["train", "--data", "d", "--out", "o"], None, False),
             "train with flags": (["train", "--data", "d", "--out", "o", "--center", "none", "--scale-factor", "0.5", "--no-auto-scale"], None, False),
             "eval with a record": (["eval", "--data", "d", "--ckpt", "c"], rec, False),
             "eval, a pose flag over the record": (["eval", "--data", "d", "--ckpt", "c", "--center-poses", "none", "--eval-mode", "all"], rec, False),
             "eval, --scale-factor 1.0 typed": (["eval", "--data", "d", "--ckpt", "c", "--scale-factor", "1.0"], rec, False),
             "--downscale-factor": (["eval", "--data", "d", "--ckpt", "c", "--downscale-factor", "2"], rec, False),
             "--downscale-factor 1 over the record": (["render", "--ckpt", "c", "--out", "o", "--data", "d", "--downscale-factor", "1"], rec, False),
             "depths=True": (["train", "--data", "d", "--out", "o", "--depth-loss", "1"], None, True),
             "depths=True with --depth-unit-scale": (["train", "--data", "d", "--out", "o", "--depth-loss", "1", "--depth-unit-scale", "0.002"], None, True),
             "depths=True with a record": (["eval", "--data", "d", "--ckpt", "c", "--depth"], rec, True)}
    out = {}
    for name, (argv, recorded, depths) in cases.items():
        kwargs, settings = trainer.capture_load_args(ap.parse_args(argv), recorded, depths)
        out[name] = {"kwargs": plain(kwargs), "settings": plain(settings), "flags": trainer.capture_flags_given(ap.parse_args(argv))}
    return out


# ------------------------------------------------------------------------------------------------ files
def look_at(eye):
    """[3,4] camera-to-world of a camera at `eye` that looks at the origin, z up (OpenGL axes: the camera looks along -z)."""
    eye = np.asarray(eye, dtype=np.float64)
    back = eye / np.linalg.norm(eye)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(back, right), back, eye], axis=1)


def poses(n):
    return [look_at([2.0 * np.cos(0.7 * i), 2.0 * np.sin(0.7 * i), 0.5 + 0.25 * i]) for i in range(n)]


def frames(n, names):
    return [{"file_path": names[i], "transform_matrix": np.vstack([c2w, [[0.0, 0.0, 0.0, 1.0]]]).tolist()} for i, c2w in enumerate(poses(n))]


def write_json(path, meta):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as fh:
        json.dump(meta, fh)


def write_files():
    """In the current directory: poses.json (w / h / camera_angle_x), nosize.json (neither), blender/ (Blender format: the size is
    in r_0.png's header), noimage/ (Blender format without an image), cap/ (a capture of equal undistorted cameras), lens/ (one with
    distortion) and run/ (a checkpoint whose rsn_run says how cap/ was read)."""
    from PIL import Image

    names = [f"./r_{i}" for i in range(5)]
    write_json("poses.json", {"camera_angle_x": 0.7, "w": W, "h": H, "frames": frames(5, names)})
    write_json("nosize.json", {"camera_angle_x": 0.7, "frames": frames(5, names)})
    for split in ("train", "test"):
        write_json(f"blender/transforms_{split}.json", {"camera_angle_x": 0.6, "frames": frames(5, names)})
    write_json("noimage/transforms_train.json", {"camera_angle_x": 0.6, "frames": frames(5, names)})
    Image.fromarray(np.zeros((7, 10, 4), dtype=np.uint8)).save("blender/r_0.png")
    for root, k1 in (("cap", 0.0), ("lens", 0.05)):
        os.makedirs(f"{root}/images")
        cap_names = [f"images/frame_{i:05d}.png" for i in range(6)]
        for name in cap_names:
            Image.fromarray(np.full((H, W, 3), 128, dtype=np.uint8)).save(f"{root}/{name}")
        write_json(f"{root}/transforms.json", {"camera_model": "OPENCV", "fl_x": 9.5, "fl_y": 9.25, "cx": 4.25, "cy": 2.75, "w": W, "h": H, "k1": k1,
                                               "frames": frames(6, cap_names)})
    trained = data.load_nerfstudio_split("cap", "train", eval_mode="all", scale_factor=0.5)
    record = {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS, "scale_factor": 0.5, "eval_mode": "all",
              "transform": trained.dataparser_transform.tolist(), "scale": trained.dataparser_scale}
    model = checkpoint.make_model(pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=8, num_importance_samples=8, num_reflect_coarse_samples=4,
                                                                     num_reflect_importance_samples=4, base_mlp_num_layers=2, base_mlp_layer_width=16), seed=0)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    checkpoint.save_checkpoint(checkpoint.checkpoint_path("run", 3), model, opt, 3, checkpoint.make_run_state(0, 1024, "f32", False, "cpu", data=record))


# ------------------------------------------------------------------------------------------------ errors through main()
MESH, TSDF, CLOUD, RENDER = (["export-mesh", "--ckpt", "c", "--out", "m.ply"], ["export-mesh", "--ckpt", "c", "--out", "m.ply", "--method", "tsdf"],
                             ["export-pointcloud", "--ckpt", "c", "--out", "c.ply"], ["render", "--ckpt", "c", "--out", "o"])
ORBIT = RENDER + ["--width", "4", "--height", "4", "--fov-x", "40"]
EVAL, TRAIN = ["eval", "--data", "d", "--ckpt", "c"], ["train", "--data", "d", "--out", "o"]
MAIN_ERRORS = [  # every line ends in an argparse error before main() asks for a GPU; the last ones could end in two and pin which
    MESH + ["--texels", "8", "--min-footprint", "0.1"], MESH + ["--texture"], ["export-mesh", "--ckpt", "c", "--out", "m.obj", "--texture", "--texels", "3"],
    ["export-mesh", "--ckpt", "c", "--out", "m.obj", "--texture", "--min-footprint", "100"],
    MESH + ["--decimate-cells", "4", "--target-faces", "10"], MESH + ["--decimate-cells", "0"], MESH + ["--target-faces", "0"],
    MESH + ["--target-faces", "10", "--resolution", "2"], MESH + ["--max-views", "2", "--trunc", "0.1", "--downscale", "2"], TSDF + ["--iso", "5"], TSDF,
    TSDF + ["--data", "d", "--poses", "p.json"], TSDF + ["--poses", "poses.json", "--trunc", "0"], TSDF + ["--poses", "poses.json", "--min-weight", "nan"],
    TSDF + ["--poses", "poses.json", "--ray-chunk", "0"], TSDF + ["--poses", "poses.json", "--max-views", "0"],
    CLOUD + ["--resolution", "0"], CLOUD + ["--edge", "-1"], CLOUD + ["--min-accumulation", "nan"], CLOUD + ["--bounds", "1", "1", "1", "0", "0", "0"],
    CLOUD + ["--ray-chunk", "0"], CLOUD + ["--chunk", "0"], CLOUD, CLOUD + ["--data", "d", "--poses", "p.json"],
    RENDER + ["--poses", "p.json", "--data", "d"], RENDER + ["--height", "4", "--fov-x", "40"], RENDER + ["--poses", "nosize.json"],
    RENDER + ["--width", "4", "--height", "4", "--fov-x", "180"], ORBIT, ORBIT + ["--path", "poses"], ORBIT + ["--radius", "2", "--frames", "0"],
    ORBIT + ["--radius", "2", "--depth-range", "5", "1"], ORBIT + ["--radius", "2", "--chunk", "0"],
    ORBIT + ["--radius", "2", "--occupancy-resolution", "8", "--occupancy-sigma", "1"], EVAL + ["--occupancy-dilate", "1", "--occupancy-bounds", "0", "0", "0", "1", "1", "1"],
    EVAL + ["--skip-empty", "--occupancy-resolution", "1"], EVAL + ["--skip-empty-samples", "--occupancy-sigma", "inf"],
    EVAL + ["--skip-empty", "--occupancy-bounds", "1", "1", "1", "0", "0", "0"],
    TRAIN + ["--primary-tan", "0"], TRAIN + ["--max-grad-norm", "0"], TRAIN + ["--multiscale", "6"], EVAL + ["--multiscale", "0"],
    EVAL + ["--depth-unit-scale", "0.001", "--depth-euclidean"], EVAL + ["--normals", "--depth"], EVAL + ["--normals-suffix", "_n", "--normals-space", "camera"],
    TRAIN + ["--multiscale", "6", "--max-grad-norm", "0", "--primary-tan", "0"], EVAL + ["--multiscale", "6", "--normals-suffix", "_n", "--depth-euclidean", "--occupancy-sigma", "1"],
    EVAL + ["--normals", "--depth", "--depth-unit-scale", "1", "--multiscale", "6"],
    MESH + ["--texels", "8", "--decimate-cells", "0", "--max-views", "2"], MESH + ["--decimate-cells", "0", "--max-views", "2"],
    TSDF + ["--iso", "5", "--trunc", "0"], TSDF + ["--poses", "nosize.json", "--downscale", "0", "--trunc", "0"],
    TSDF + ["--poses", "poses.json", "--downscale", "0", "--trunc", "0"], CLOUD + ["--chunk", "0", "--poses", "nosize.json"],
    RENDER + ["--poses", "poses.json", "--fov-x", "180", "--chunk", "0", "--occupancy-sigma", "1"],
]


def no_gpu():
    raise AssertionError("this command line reached main()'s test for a GPU: it does not belong in the record")


def main_errors():
    with mock.patch.object(torch.cuda, "is_available", no_gpu):
        return {" ".join(argv): error_of(trainer.main, argv) for argv in MAIN_ERRORS}


# ------------------------------------------------------------------------------------------------ resolved values
CAP_MESH = ["export-mesh", "--method", "tsdf", "--ckpt", "run", "--out", "m.ply", "--data", "cap"]
RESOLVED = {
    "resolve_render_args": [RENDER + ["--poses", "poses.json"], RENDER + ["--poses", "poses.json", "--interpolate", "1", "--scale-factor", "0.5", "--width", "16"],
                            RENDER + ["--data", "blender", "--path", "orbit", "--frames", "3"], RENDER + ["--data", "blender", "--split", "train", "--path", "poses"],
                            RENDER + ["--data", "blender", "--radius", "3", "--elevation", "10", "--frames", "2", "--fov-x", "50"],
                            ["render", "--ckpt", "run", "--out", "o", "--data", "cap"],
                            ["render", "--ckpt", "run", "--out", "o", "--data", "cap", "--path", "orbit", "--frames", "3"],
                            ["render", "--ckpt", "run", "--out", "o", "--data", "cap", "--path", "orbit", "--frames", "2", "--fov-x", "50"],
                            ["render", "--ckpt", "run", "--out", "o", "--data", "lens", "--eval-mode", "all"],
                            RENDER + ["--poses", "nosize.json"], RENDER + ["--data", "noimage", "--split", "train"], RENDER + ["--data", "nowhere"],
                            ["render", "--ckpt", "run", "--out", "o", "--data", "cap", "--interpolate", "1"],
                            ["render", "--ckpt", "run", "--out", "o", "--data", "cap", "--fov-x", "40"],
                            ["render", "--ckpt", "nowhere", "--out", "o", "--data", "cap"]],
    "resolve_export_cameras": [MESH, CAP_MESH + ["--max-views", "2", "--downscale", "2"], CAP_MESH, CAP_MESH + ["--max-views", "9", "--downscale", "16"],
                               TSDF + ["--poses", "poses.json", "--max-views", "2", "--downscale", "2"],
                               TSDF + ["--data", "blender", "--max-views", "2", "--downscale", "2", "--scale-factor", "0.5"],
                               TSDF + ["--data", "blender", "--split", "test", "--max-views", "3", "--downscale", "3"],
                               TSDF + ["--poses", "nosize.json"], TSDF + ["--data", "noimage"], TSDF + ["--poses", "poses.json", "--downscale", "0"],
                               TSDF + ["--poses", "nosize.json", "--downscale", "0"], CAP_MESH + ["--downscale", "0"], CAP_MESH + ["--max-views", "0"],
                               ["export-mesh", "--method", "tsdf", "--ckpt", "run", "--out", "m.ply", "--data", "lens"], TSDF + ["--data", "nowhere"]],
    "resolve_pointcloud_args": [CLOUD + ["--poses", "poses.json", "--max-views", "2", "--downscale", "2"],
                                CLOUD + ["--data", "blender", "--max-views", "2", "--downscale", "2", "--no-edge", "--no-thin", "--bounds", "-1", "-1", "-1", "1", "1", "1"],
                                ["export-pointcloud", "--ckpt", "run", "--out", "c.ply", "--data", "cap", "--max-views", "2", "--downscale", "2"],
                                CLOUD + ["--poses", "nosize.json"], CLOUD + ["--poses", "poses.json", "--downscale", "0"]],
    "resolve_occupancy_args": [EVAL, EVAL + ["--skip-empty"], EVAL + OCCUPANCY_FLAGS],
    "resolve_decimate_args": [MESH, MESH + ["--decimate-cells", "4"], MESH + ["--target-faces", "10"]],
}
SCENE_ERRORS = [["train", "--data", "blender", "--out", "o", "--orientation", "none", "--downscale-factor", "2"], ["train", "--data", "nowhere", "--out", "o"],
                ["eval", "--data", "cap", "--ckpt", "run", "--downscale-factor", "2"]]


def resolved():
    """The value each resolver returns for each command line above, or {"error": the argparse error's text}; and the errors of
    load_scene that a `train` or `eval` line ends with after main()'s test for a GPU."""
    ap = trainer.build_parser()
    out = {}
    for name, lines in RESOLVED.items():
        for argv in lines:
            out[f"{name}: {' '.join(argv)}"] = value_or_error(getattr(trainer, name), ap, ap.parse_args(argv))
    for argv in SCENE_ERRORS:
        args = ap.parse_args(argv)
        recorded = checkpoint.read_run_state(args.ckpt) if args.command == "eval" else None
        out[f"load_scene: {' '.join(argv)}"] = {"error": error_of(trainer.load_scene, ap, args, "train", recorded)}
    return out


# ------------------------------------------------------------------------------------------------ what main() hands to train()
class Scene:
    """What main() reads of a loaded scene."""
    num_images, width, height, fx, cameras, depths = 3, 8, 8, 9.5, None, ()


def train_calls():
    """The arguments train() gets from main() for the minimal and the full `train` line (and what main() prints on the way), with the
    GPU test, the scene loader, the checkpoint reader and train() itself replaced: nothing is loaded and nothing runs."""
    import inspect

    signature = inspect.signature(trainer.train)
    minimal, more = PARSES["train"]
    out = {}
    for which, argv in (("minimal", minimal), ("full", minimal + more)):
        printed = io.StringIO()
        with mock.patch.object(torch.cuda, "is_available", lambda: True), mock.patch.object(trainer, "read_run_state", lambda path: None), \
                mock.patch.object(trainer, "load_scene", lambda *a, **k: (Scene(), {"format": "stand-in"})), \
                mock.patch.object(trainer, "train") as train, contextlib.redirect_stdout(printed):
            assert trainer.main(argv) == 0
        (args, kwargs), = train.call_args_list
        bound = signature.bind(*args, **kwargs)
        bound.apply_defaults()
        assert isinstance(bound.arguments.pop("scene"), Scene) and bound.arguments.pop("log") is print
        out[which] = {"arguments": plain(dict(bound.arguments)), "printed": printed.getvalue()}
    return out


def record():
    """Every group of the record.  Writes its files into the current directory, which the caller has made an empty one: every path
    in a message is then a relative one."""
    write_files()
    return {"parses": parses(), "run_state": {"make_run_state": run_states(), "_resolve_run_settings": resolved_settings()},
            "capture_args": capture_args(), "main_errors": main_errors(), "resolved": resolved(), "train_calls": train_calls()}


def dump(rec, fh):
    json.dump(rec, fh, indent=0, sort_keys=True)
    fh.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "cli_cases.json"))
    a = ap.parse_args()
    out = os.path.abspath(a.out)
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        rec = record()
    with open(out, "w") as fh:
        dump(rec, fh)
    print(f"wrote {out}")
