"""Checkpoints in nerfstudio's layout (step-{step:09d}.ckpt: step / pipeline / optimizers / scalers, plus the trainer's `rsn_run`):
writing, finding and loading them, for the trainer (which re-exports these names) and for every tool that opens one."""
from __future__ import annotations

import os
import re
from typing import Callable, Dict, NamedTuple, Optional

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


def _when_set(v):
    return None if v is None else float(v)


def _when_true(v):
    return True if v else None


def _above_one(v):
    return int(v) if v is not None and int(v) > 1 else None


def _coefficient(v):
    return float(v) if v is not None and float(v) != 0.0 else None


def _as_it_is(v):
    return v


class RunSetting(NamedTuple):
    default: object  # what a fresh run gets when it is not told (None: off, or the model's own)
    record: Callable  # the value -> what `rsn_run` holds for it; None: the key is left out
    term: Optional[str] = None  # the part of the run it belongs to; a loss term's further settings are recorded only with a coefficient


PRIMARY_RAYS = "primary rays"
# The settings of a run, each stated once: `train` takes them by these names, --resume restores them, make_run_state records them
# (in this order) and the line that starts a run prints them.  rays / mma / seed: reflect_sampling_nerf_config.py:36-41.
# An unguarded, single-scale run without the opt-in loss terms on a Blender-format scene records the first four alone: the keys
# its checkpoints always had.
RUN_SETTINGS = {
    "rays": RunSetting(1024, int),
    "mma": RunSetting("f32", str),
    "seed": RunSetting(0, int),
    "deterministic": RunSetting(None, bool),
    "max_grad_norm": RunSetting(None, _when_set),  # the optimiser's guard
    "skip_nonfinite": RunSetting(None, _when_true),
    "multiscale": RunSetting(1, _above_one),  # the number of pyramid levels the rays are drawn from
    "distortion_loss": RunSetting(None, _coefficient, "distortion"),  # the opt-in distortion term, fine / coarse level
    "distortion_loss_coarse": RunSetting(None, _coefficient, "distortion"),
    "depth_loss": RunSetting(None, _coefficient, "depth"),  # the opt-in depth term
    "depth_loss_coarse": RunSetting(None, _coefficient, "depth"),
    "depth_sigma": RunSetting(None, _when_set, "depth"),
    "depth_euclidean": RunSetting(None, _when_true, "depth"),
    "near": RunSetting(None, _as_it_is, PRIMARY_RAYS),  # the collider planes
    "far": RunSetting(None, _as_it_is, PRIMARY_RAYS),
    "primary_spacing": RunSetting(None, _as_it_is, PRIMARY_RAYS),  # the coarse sampler of the primary rays
    "primary_tan": RunSetting(None, _as_it_is, PRIMARY_RAYS),
}
COEFFICIENTS = tuple(k for k, s in RUN_SETTINGS.items() if s.record is _coefficient)
RAY_KEYS = tuple(k for k, s in RUN_SETTINGS.items() if s.term == PRIMARY_RAYS)
LOSS_TERMS = {RUN_SETTINGS[k].term for k in COEFFICIENTS}
PRIMARY_SPACINGS = ("uniform", "reciprocal")


def recorded_settings(settings: dict) -> dict:
    """The entries of RUN_SETTINGS that `rsn_run` holds for a run with these settings, in the table's order: each by its own rule,
    and a loss term's further settings only beside one of its coefficients.  Of the optional ones an absent name counts as None;
    KeyError for a name the table does not have."""
    unknown = sorted(set(settings) - set(RUN_SETTINGS))
    if unknown:
        raise KeyError(f"unknown run settings {unknown}")
    out, terms_on = {}, set()
    for name, s in RUN_SETTINGS.items():
        v = s.record(settings.get(name))
        if v is None:
            continue
        if name in COEFFICIENTS:
            terms_on.add(s.term)
        if s.term not in LOSS_TERMS or s.term in terms_on:
            out[name] = v
    return out


def make_run_state(seed: int, rays: int, mma: str, deterministic: bool, device, data: Optional[dict] = None, **settings) -> dict:
    """What a checkpoint needs beyond model, optimiser and step for `train(resume=...)` to continue with the uninterrupted run's
    bits: the run's settings and the two torch generators as they stand now (i.e. after the checkpoint's step; the CUDA generator's
    seed and offset live on the host, reading them waits for nothing).  cuda_rng_state is None for a device without one.
    settings: the further entries of RUN_SETTINGS, each by its own name and recorded by its own rule there (recorded_settings): a
    run that sets none of them has the keys it always had.  max_grad_norm when set and skip_nonfinite when true; multiscale above
    1; a coefficient -- distortion_loss / distortion_loss_coarse, depth_loss / depth_loss_coarse -- when set and not 0, and only
    with a depth coefficient depth_sigma (when set) and depth_euclidean (when true); near / far / primary_spacing / primary_tan
    when not None.  data: how a capture was read (format, orientation, center, auto_scale, scale_factor, train_split_fraction,
    eval_mode, and the transform [3][4] and scale that were applied), recorded when not None; a Blender-format run has none."""
    dev = torch.device(device)
    state = {"version": RUN_STATE_VERSION, "cuda_rng_state": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None,
             "cpu_rng_state": torch.get_rng_state(), **recorded_settings(dict(settings, seed=seed, rays=rays, mma=mma, deterministic=deterministic))}
    if data is not None:
        state["data"] = data
    return state


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
