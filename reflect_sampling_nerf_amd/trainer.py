"""Standalone training and evaluation on Blender-format scenes, without nerfstudio.

    python -m reflect_sampling_nerf_amd.trainer train --data DIR --out DIR [--steps N] [--rays 1024] [--mma f32|bf16x6|bf16]
    python -m reflect_sampling_nerf_amd.trainer eval --data DIR --ckpt FILE [--split test] [--out metrics.json]

`train` is the reference's `ns-train reflect-sampling-nerf --data DIR` loop on this package's own pieces: the reference
Model config (ReflectSamplingNeRFModelConfig defaults), RayDataManager batches (1024 rays, reflect_sampling_nerf_config.py:36-41),
parallel.train_step (50-step loss warm-up included) and FusedRAdam with the reference's schedule (config.py:50-53).  Checkpoints
use nerfstudio's layout (step-{step:09d}.ckpt holding step / pipeline / optimizers / scalers).  `eval` renders held-out
views in the reference's 1024-ray chunks and writes an ns-eval-shaped JSON: psnr, coarse_psnr, fine_psnr
(get_image_metrics_and_images) and fine_ssim (metrics.ssim of the clipped mid_reflect_fine render, model.py:468-479).
fine_lpips is not computed: it needs pretrained network weights that are not part of this package.
Resuming from a checkpoint and multi-GPU training are not offered here.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Callable, Dict, Optional

import numpy as np
import torch

METHOD_NAME = "reflect-sampling-nerf"
MMA_CHOICES = ("f32", "bf16x6", "bf16")
EVAL_CHUNK = 1024  # reflect_sampling_nerf_config.py:41 eval_num_rays_per_chunk
LPIPS_NOTE = "fine_lpips not computed: LPIPS needs pretrained network weights that are not shipped with this package"


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m reflect_sampling_nerf_amd.trainer", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)
    tr = sub.add_parser("train", help="train on the train split of a Blender-format scene")
    tr.add_argument("--data", required=True, help="scene directory with transforms_train.json")
    tr.add_argument("--out", required=True, help="directory for step-*.ckpt")
    tr.add_argument("--steps", type=int, default=100000, help="training iterations (reference max_num_iterations)")
    tr.add_argument("--rays", type=int, default=1024, help="rays per batch")
    tr.add_argument("--mma", choices=MMA_CHOICES, default="f32", help="matrix-core arithmetic of the field kernels")
    tr.add_argument("--save-every", type=int, default=1000, help="checkpoint interval in steps")
    tr.add_argument("--log-every", type=int, default=100, help="loss read-back interval in steps (0: never)")
    tr.add_argument("--seed", type=int, default=0, help="model initialisation and ray sampling seed")
    tr.add_argument("--deterministic", action="store_true",
                    help="bit-reproducible run: weight gradients reduced in a fixed order (slower flush, one 68 MB workspace)")
    tr.add_argument("--scale-factor", type=float, default=1.0, help="BlenderDataParser scale_factor")
    ev = sub.add_parser("eval", help="score a checkpoint on held-out views")
    ev.add_argument("--data", required=True, help="scene directory with transforms_{split}.json")
    ev.add_argument("--ckpt", required=True, help="step-*.ckpt written by `train` (or by ns-train)")
    ev.add_argument("--split", default="test")
    ev.add_argument("--max-images", type=int, default=None, help="score only the first N views")
    ev.add_argument("--out", default="metrics.json", help="output JSON")
    ev.add_argument("--save-images", default=None, help="directory for rendered ground truth | coarse | fine panels")
    ev.add_argument("--scale-factor", type=float, default=1.0, help="BlenderDataParser scale_factor")
    return ap


# ------------------------------------------------------------------------------------------------ model and checkpoints
def make_model(model_config=None, seed: int = 0):
    """A ReflectSamplingNeRFModel (reference defaults unless `model_config` is given), initialised from `seed`, on the CPU."""
    from .reflect_sampling_nerf_model import ReflectSamplingNeRFModelConfig

    cfg = model_config if model_config is not None else ReflectSamplingNeRFModelConfig()
    torch.manual_seed(seed)
    return cfg.setup(scene_box=None, num_train_data=1)


def checkpoint_path(out_dir: str, step: int) -> str:
    return os.path.join(out_dir, f"step-{step:09d}.ckpt")


def save_checkpoint(path: str, model, optimizer, step: int) -> str:
    """nerfstudio's trainer layout: the pipeline's state dict is the model's under the `_model.` prefix."""
    pipeline = {"_model." + k: v.detach().cpu() for k, v in model.state_dict().items()}
    opt = optimizer.state_dict()
    opt = {"state": {i: {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
                     for i, st in opt["state"].items()}, "param_groups": opt["param_groups"]}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({"step": int(step), "pipeline": pipeline, "optimizers": {"fields": opt}, "scalers": {}}, path + ".tmp")
    os.replace(path + ".tmp", path)
    return path


def config_for_checkpoint(pipeline_state: Dict[str, torch.Tensor], model_config=None):
    """The model config to load `pipeline_state` into: `model_config` if given, else the reference defaults with the trunk
    depth and width read off the checkpoint's `_model.field.mlp_base.layers.*` tensors."""
    from .reflect_sampling_nerf_model import ReflectSamplingNeRFModelConfig

    if model_config is not None:
        return model_config
    prefix = "_model.field.mlp_base.layers."
    layers = {int(k[len(prefix):].split(".")[0]) for k in pipeline_state if k.startswith(prefix)}
    if not layers:
        return ReflectSamplingNeRFModelConfig()
    width = int(pipeline_state[prefix + "0.weight"].shape[0])
    return ReflectSamplingNeRFModelConfig(base_mlp_num_layers=max(layers) + 1, base_mlp_layer_width=width)


class _Pipeline(torch.nn.Module):
    """The parent the checkpoint's `_model.` keys belong to (nerfstudio's VanillaPipeline)."""

    def __init__(self, model):
        super().__init__()
        self._model = model


def load_checkpoint(path: str, model_config=None, device="cuda:0"):
    """-> (model in eval mode on `device`, checkpoint step).  Strict key check: the reference's own pipeline checkpoints
    load too (their torchmetrics entries, `_model.lpips.*`, are dropped by the Model's load pre-hook)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    state = ckpt["pipeline"]
    model = make_model(config_for_checkpoint(state, model_config))
    _Pipeline(model).load_state_dict(state, strict=True)
    return model.to(device).eval(), int(ckpt.get("step", -1))


# ------------------------------------------------------------------------------------------------ train
def train(scene, out_dir: str, steps: int = 100000, rays: int = 1024, mma: str = "f32", save_every: int = 1000,
          log_every: int = 100, seed: int = 0, device="cuda:0", model_config=None,
          log: Optional[Callable[[str], None]] = print, deterministic: Optional[bool] = None) -> str:
    """Train on `scene` (a data.BlenderScene) for `steps` iterations; returns the path of the last checkpoint.  Checkpoints
    at every step > 0 divisible by save_every and after the last step (nerfstudio's trainer does the same).  The loss is
    read back only every log_every steps: the iterations in between never wait for the GPU.  deterministic: Model.set_deterministic
    (None: the model's default, i.e. the environment's RSN_DETERMINISTIC); the line that starts the run records it."""
    from .data import RayDataManager
    from .parallel import train_step
    from .train_ops import FusedRAdam

    if mma not in MMA_CHOICES:
        raise ValueError(f"mma must be one of {MMA_CHOICES}, got {mma!r}")
    if steps < 1:
        raise ValueError(f"steps must be >= 1, got {steps}")
    dev = torch.device(device)
    model = make_model(model_config, seed).to(dev).train()
    model.field.set_mma_mode(mma)
    if deterministic is not None:
        model.set_deterministic(deterministic)
    if log is not None:
        log(f"train: steps {steps} rays {rays} mma {mma} seed {seed} deterministic {model.deterministic}")
    dm = RayDataManager(scene, dev, num_rays_per_batch=rays, seed=seed)
    params = model.get_param_groups()["fields"]
    optimizer = FusedRAdam(params, lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)  # config.py:50-53
    last = None
    t0 = time.time()
    for step in range(steps):
        ray_bundle, batch = dm.next_train(step)
        loss = train_step(model, ray_bundle, batch, optimizer, None, step)
        if log is not None and log_every and (step % log_every == 0 or step == steps - 1):
            log(f"step {step:7d}  loss {float(loss):.6f}  lr {optimizer.current_lr():.3e}  {time.time() - t0:8.1f} s")
        if (save_every and step > 0 and step % save_every == 0) or step == steps - 1:
            last = save_checkpoint(checkpoint_path(out_dir, step), model, optimizer, step)
            if log is not None:
                log(f"saved {last}")
    return last


# ------------------------------------------------------------------------------------------------ eval
def _white(image: torch.Tensor) -> torch.Tensor:
    return image[..., :3] * image[..., 3:] + (1.0 - image[..., 3:]) if image.shape[-1] == 4 else image


def evaluate(scene, ckpt: str, max_images: Optional[int] = None, save_images: Optional[str] = None, device="cuda:0",
             model_config=None) -> dict:
    """Score the checkpoint on every view of `scene` (a data.BlenderScene); -> ns-eval-shaped dict."""
    from . import metrics
    from .data import RayDataManager

    dev = torch.device(device)
    model, step = load_checkpoint(ckpt, model_config, dev)
    model.config.eval_num_rays_per_chunk = EVAL_CHUNK
    dm = RayDataManager(scene, dev)
    n = scene.num_images if max_images is None else min(int(max_images), scene.num_images)
    if save_images:
        os.makedirs(save_images, exist_ok=True)
    per_image = []
    for i in range(n):
        torch.cuda.synchronize(dev)
        t0 = time.time()
        outputs = model.get_outputs_for_camera_ray_bundle(dm.camera_ray_bundle(i))
        gt = dm.image(i)
        m, images = model.get_image_metrics_and_images(outputs, {"image": gt})
        m = dict(m)
        m["fine_ssim"] = float(metrics.ssim(torch.clip(outputs["mid_reflect_fine"], 0.0, 1.0), _white(gt)))
        dt = time.time() - t0
        m["num_rays_per_sec"] = scene.height * scene.width / dt
        m["fps"] = 1.0 / dt
        per_image.append({"image": i, **m})
        if save_images:
            from PIL import Image

            panel = (images["img"].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
            Image.fromarray(panel).save(os.path.join(save_images, f"{i:04d}_img.png"))
    keys = [k for k in per_image[0] if k != "image"] if per_image else []
    results = {}
    for k in keys:
        v = np.array([p[k] for p in per_image], dtype=np.float64)
        results[k] = float(v.mean())
        results[k + "_std"] = float(v.std(ddof=1)) if len(v) > 1 else 0.0  # torch.std_mean (ns-eval): unbiased
    return {"experiment_name": os.path.basename(os.path.dirname(os.path.abspath(ckpt))), "method_name": METHOD_NAME,
            "checkpoint": ckpt, "step": step, "results": results, "not_computed": {"fine_lpips": LPIPS_NOTE},
            "per_image": per_image}


# ------------------------------------------------------------------------------------------------ CLI
def main(argv=None) -> int:
    from .data import load_blender_split

    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        print("reflect_sampling_nerf_amd.trainer needs a GPU (the HIP kernels have no CPU path)", file=sys.stderr)
        return 2
    if args.command == "train":
        scene = load_blender_split(args.data, "train", args.scale_factor)
        print(f"{args.data}: {scene.num_images} train images {scene.width} x {scene.height}, focal {scene.fx:.3f}")
        train(scene, args.out, steps=args.steps, rays=args.rays, mma=args.mma, save_every=args.save_every,
              log_every=args.log_every, seed=args.seed, deterministic=True if args.deterministic else None)
        return 0
    scene = load_blender_split(args.data, args.split, args.scale_factor)
    res = evaluate(scene, args.ckpt, max_images=args.max_images, save_images=args.save_images)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=2)
    r = res["results"]
    print(" ".join(f"{k} {r[k]:.4f}" for k in ("psnr", "coarse_psnr", "fine_psnr", "fine_ssim") if k in r
                   and not math.isnan(r[k])) + f"  ({len(res['per_image'])} images) -> {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
