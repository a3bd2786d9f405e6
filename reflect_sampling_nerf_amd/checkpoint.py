"""Checkpoints in nerfstudio's layout (step-{step:09d}.ckpt: step / pipeline / optimizers / scalers, plus the trainer's `rsn_run`):
writing, finding and loading them, for the trainer (which re-exports these names) and for every tool that opens one."""
from __future__ import annotations

import os
import re
from typing import Dict, Optional

import torch

from ._host import replacing

RUN_STATE_KEY = "rsn_run"  # the trainer's own fifth checkpoint key; nerfstudio's loader ignores it
RUN_STATE_VERSION = 1


def make_model(model_config=None, seed: int = 0):
    """A ReflectSamplingNeRFModel (reference defaults unless `model_config` is given), initialised from `seed`, on the CPU."""
    from .reflect_sampling_nerf_model import ReflectSamplingNeRFModelConfig

    cfg = model_config if model_config is not None else ReflectSamplingNeRFModelConfig()
    torch.manual_seed(seed)
    return cfg.setup(scene_box=None, num_train_data=1)


def checkpoint_path(out_dir: str, step: int) -> str:
    return os.path.join(out_dir, f"step-{step:09d}.ckpt")


_STEP_CKPT = re.compile(r"^step-(\d+)\.ckpt$")


def latest_checkpoint(run_dir: str) -> str:
    """The step-*.ckpt of the highest step in `run_dir` (nerfstudio's --load-dir rule); FileNotFoundError when there is none."""
    best = None
    for name in os.listdir(run_dir):
        m = _STEP_CKPT.match(name)  # a step-*.ckpt.tmp is a save that never finished
        if m and (best is None or int(m.group(1)) > best[0]):
            best = (int(m.group(1)), name)
    if best is None:
        raise FileNotFoundError(f"no step-*.ckpt in {run_dir}")
    return os.path.join(run_dir, best[1])


def resolve_checkpoint(path: str) -> str:
    """`path` itself, or the latest checkpoint of the run directory `path`."""
    return latest_checkpoint(path) if os.path.isdir(path) else path


def make_run_state(seed: int, rays: int, mma: str, deterministic: bool, device, max_grad_norm: Optional[float] = None,
                   skip_nonfinite: Optional[bool] = None, multiscale: Optional[int] = None, distortion_loss: Optional[float] = None,
                   distortion_loss_coarse: Optional[float] = None, rays_and_data: Optional[dict] = None,
                   depth: Optional[dict] = None) -> dict:
    """What a checkpoint needs beyond model, optimiser and step for `train(resume=...)` to continue with the uninterrupted run's
    bits: the run's settings and the two torch generators as they stand now (i.e. after the checkpoint's step; the CUDA generator's
    seed and offset live on the host, reading them waits for nothing).  cuda_rng_state is None for a device without one.
    max_grad_norm / skip_nonfinite (the optimiser's guard) are recorded only when set: an unguarded run's entry has the keys it
    always had.  Likewise multiscale (the number of pyramid levels the rays are drawn from): only when above 1, and distortion_loss /
    distortion_loss_coarse (the coefficients of the opt-in distortion term): only when set and not 0.  rays_and_data: the entries
    of RAY_KEYS ("near", "far": the collider planes; "primary_spacing", "primary_tan": the coarse sampler of the primary rays) and
    "data" (how a capture was read: format, orientation, center, auto_scale, scale_factor, train_split_fraction, eval_mode, and the
    transform [3][4] and scale that were applied) that are not None are recorded; a Blender-format run with its defaults has none.
    depth: the settings of the opt-in depth term, DEPTH_RUN_KEYS: "depth_loss" / "depth_loss_coarse" (the coefficients) are recorded
    when set and not 0, and only with one of them "depth_sigma" (when set) and "depth_euclidean" (when true); a run without the term
    records none of them."""
    dev = torch.device(device)
    state = {"version": RUN_STATE_VERSION, "seed": int(seed), "rays": int(rays), "mma": str(mma), "deterministic": bool(deterministic),
             "cuda_rng_state": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None,
             "cpu_rng_state": torch.get_rng_state()}
    if max_grad_norm is not None:
        state["max_grad_norm"] = float(max_grad_norm)
    if skip_nonfinite:
        state["skip_nonfinite"] = True
    if multiscale is not None and int(multiscale) > 1:
        state["multiscale"] = int(multiscale)
    for key, coef in (("distortion_loss", distortion_loss), ("distortion_loss_coarse", distortion_loss_coarse)):
        if coef is not None and float(coef) != 0.0:
            state[key] = float(coef)
    depth = depth or {}
    if set(depth) - set(DEPTH_RUN_KEYS):
        raise KeyError(f"depth: unknown entries {sorted(set(depth) - set(DEPTH_RUN_KEYS))}")
    coefs = {k: float(depth[k]) for k in ("depth_loss", "depth_loss_coarse") if depth.get(k) is not None and float(depth[k]) != 0.0}
    if coefs:
        state.update(coefs)
        if depth.get("depth_sigma") is not None:
            state["depth_sigma"] = float(depth["depth_sigma"])
        if depth.get("depth_euclidean"):
            state["depth_euclidean"] = True
    for key, v in (rays_and_data or {}).items():
        if key not in RAY_KEYS + ("data",):
            raise KeyError(f"rays_and_data: unknown entry {key!r}")
        if v is not None:
            state[key] = v
    return state


RAY_KEYS = ("near", "far", "primary_spacing", "primary_tan")
DEPTH_RUN_KEYS = ("depth_loss", "depth_loss_coarse", "depth_sigma", "depth_euclidean")
PRIMARY_SPACINGS = ("uniform", "reciprocal")


def read_run_state(path: str) -> Optional[dict]:
    """The `rsn_run` entry of a step-*.ckpt (or of the newest one of a run directory); None for a checkpoint without one."""
    return torch.load(resolve_checkpoint(path), map_location="cpu", weights_only=False).get(RUN_STATE_KEY)


def config_with_planes(config, near: Optional[float] = None, far: Optional[float] = None):
    """`config` itself when both are None, else a copy whose collider_params hold the given planes (the other one as it was)."""
    if near is None and far is None:
        return config
    import copy

    planes = dict(config.collider_params)
    if near is not None:
        planes["near_plane"] = float(near)
    if far is not None:
        planes["far_plane"] = float(far)
    if not planes["far_plane"] > planes["near_plane"] >= 0.0:
        raise ValueError(f"near {planes['near_plane']} far {planes['far_plane']}: need 0 <= near < far")
    config = copy.copy(config)
    config.collider_params = planes
    return config


def set_primary_sampler(model, spacing: Optional[str] = None, tan: Optional[float] = None) -> None:
    """The coarse sampler of the primary rays: None or "uniform" leaves model.sampler_uniform as the model built it; "reciprocal"
    replaces it by ReciprocalSampler(tan) with the same sample count (spacing s(t) = t / (1/tan + t): fine near the camera, coarse
    far away, for a far plane an unbounded scene needs).  The samplers, the training graph and the eval path read the spacing and tan
    from that object's spec."""
    if spacing not in (None,) + PRIMARY_SPACINGS:
        raise ValueError(f"primary_spacing = {spacing!r}: choose from {', '.join(PRIMARY_SPACINGS)}")
    if spacing == "reciprocal":
        from .reflect_sampling_nerf_components import ReciprocalSampler

        tan = 1.0 if tan is None else float(tan)
        if not tan > 0.0:
            raise ValueError(f"primary_tan = {tan}: need a value above 0")
        model.sampler_uniform = ReciprocalSampler(tan=tan, num_samples=model.config.num_coarse_samples)


def save_checkpoint(path: str, model, optimizer, step: int, run_state: Optional[dict] = None) -> str:
    """nerfstudio's trainer layout: the pipeline's state dict is the model's under the `_model.` prefix.  run_state
    (make_run_state) goes under a fifth key, `rsn_run`, only when given."""
    pipeline = {"_model." + k: v.detach().cpu() for k, v in model.state_dict().items()}
    opt = optimizer.state_dict()
    opt = {"state": {i: {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in st.items()}
                     for i, st in opt["state"].items()}, "param_groups": opt["param_groups"]}
    ckpt = {"step": int(step), "pipeline": pipeline, "optimizers": {"fields": opt}, "scalers": {}}
    if run_state is not None:
        ckpt[RUN_STATE_KEY] = run_state
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with replacing(path) as tmp:
        torch.save(ckpt, tmp)
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


def _load_pipeline(path: str, model_config=None, rays: Optional[dict] = None, ckpt: Optional[dict] = None):
    """-> (model on the CPU with the checkpoint's `pipeline` loaded under strict key checking, the checkpoint dict).  The collider
    planes and the primary rays' coarse sampler that the run recorded (RAY_KEYS of `rsn_run`) are set on the model: every tool that
    opens the checkpoint casts its rays the way the run did.  A checkpoint without them gets the config's.  rays: entries of
    RAY_KEYS that take the place of the recorded ones (None entries do not).  ckpt: the file's content when the caller has read it."""
    if ckpt is None:
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    state = ckpt["pipeline"]
    run = dict(ckpt.get(RUN_STATE_KEY) or {})
    run.update({k: v for k, v in (rays or {}).items() if v is not None})
    model = make_model(config_with_planes(config_for_checkpoint(state, model_config), run.get("near"), run.get("far")))
    set_primary_sampler(model, run.get("primary_spacing"), run.get("primary_tan"))
    _Pipeline(model).load_state_dict(state, strict=True)
    return model, ckpt


def load_checkpoint(path: str, model_config=None, device="cuda:0"):
    """-> (model in eval mode on `device`, checkpoint step).  Strict key check: the reference's own pipeline checkpoints
    load too (their torchmetrics entries, `_model.lpips.*`, are dropped by the Model's load pre-hook)."""
    model, ckpt = _load_pipeline(path, model_config)
    return model.to(device).eval(), int(ckpt.get("step", -1))


def open_checkpoint(ckpt: str, model_config=None, device="cuda:0", mma: Optional[str] = None):
    """A step-*.ckpt, or a run directory (its newest) -> (the file's path, model in eval mode on `device`, checkpoint step).
    mma: the field's matrix-core arithmetic (None: as the model sets it up)."""
    path = resolve_checkpoint(ckpt)
    model, step = load_checkpoint(path, model_config, device)
    if mma is not None:
        model.field.set_mma_mode(mma)
    return path, model, step
