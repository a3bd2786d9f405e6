"""ReflectSamplingNeRFModel on MI355X: the reference's Model hooks, config fields and output keys
(reflect_sampling_nerf_model.py:38-430), with get_outputs driven through librsn_hip.so.

get_outputs (reference model.py:142-344) becomes a fixed sequence of asynchronous kernel launches on the
current stream -- samplers, the fused field kernel, per-ray compositing, device-side stable compaction of
the reflected rays (dynamic M read from device memory by the later launches) -- with NO host sync: the one
output whose SHAPE depends on M (`depth_reflect_fine`, [M, 1]) is materialised on first use (ops.LazyOutputs).
The reference's debug prints / six syncs (model.py:230,263-265,342) are not reproduced.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Type

import torch
from torch import Tensor, nn
from torch.nn import Parameter

from . import ops
from .nerfstudio_compat import Model, ModelConfig
from .reflect_sampling_nerf_components import (
    IntegratedSHEncoding,
    NeRFEncoding,
    PDFSampler,
    ReciprocalSampler,
    UniformSampler,
)
from .reflect_sampling_nerf_field import ReflectSamplingNeRFNerfField

_LOSS_COEFFICIENTS = {
    "loss_low_coarse": 1e-1,
    "loss_low_fine": 1e-1,
    "loss_mid_coarse": 1.0,
    "loss_mid_fine": 1.0,
    "loss_reflect_low_coarse": 1e-1,
    "loss_reflect_low_fine": 1e-1,
    "loss_reflect_mid_coarse": 1.0,
    "loss_reflect_mid_fine": 1.0,
    "predicted_normal_loss_coarse": 3e-5,
    "predicted_normal_loss_fine": 3e-4,
    "orientation_loss_coarse": 1e-2,
    "orientation_loss_fine": 1e-1,
}


@dataclass
class ReflectSamplingNeRFModelConfig(ModelConfig):
    """Same field names and defaults as the reference config (model.py:38-75)."""

    num_coarse_samples: int = 128
    num_importance_samples: int = 128
    num_reflect_coarse_samples: int = 64
    num_reflect_importance_samples: int = 64
    loss_coefficients: Dict[str, float] = field(default_factory=lambda: dict(_LOSS_COEFFICIENTS))
    enable_temporal_distortion: bool = False
    temporal_distortion_params: Dict[str, Any] = field(default_factory=lambda: {"kind": "dnerf"})
    # Field size knobs (constructor arguments of the reference Field, field.py:40-41).  The reference Model
    # always builds the default 8 x 256 Field; BASELINE.json's configs turn these two.
    base_mlp_num_layers: int = 8
    base_mlp_layer_width: int = 256
    _target: Type = field(default_factory=lambda: ReflectSamplingNeRFModel)


class ReflectSamplingNeRFModel(Model):
    config: ReflectSamplingNeRFModelConfig

    def __init__(self, config: ReflectSamplingNeRFModelConfig, **kwargs) -> None:
        self.field = None
        assert config.collider_params is not None, "MipNeRF model requires bounding box collider parameters."
        super().__init__(config=config, **kwargs)
        assert self.config.collider_params is not None, "mip-NeRF requires collider parameters to be set."

    # ------------------------------------------------------------------ construction (model.py:93-132)
    def populate_modules(self):
        super().populate_modules()
        position_encoding = NeRFEncoding(in_dim=3, num_frequencies=16, min_freq_exp=0.0, max_freq_exp=16.0,
                                         include_input=True)
        direction_encoding = IntegratedSHEncoding()
        self.field = ReflectSamplingNeRFNerfField(
            position_encoding=position_encoding,
            direction_encoding=direction_encoding,
            base_mlp_num_layers=getattr(self.config, "base_mlp_num_layers", 8),
            base_mlp_layer_width=getattr(self.config, "base_mlp_layer_width", 256),
        )
        self.sampler_uniform = UniformSampler(num_samples=self.config.num_coarse_samples)
        self.sampler_pdf = PDFSampler(num_samples=self.config.num_importance_samples, include_original=False)
        self.sampler_reciprocal = ReciprocalSampler(num_samples=self.config.num_reflect_coarse_samples, tan=0.25)
        self.sampler_reflect_pdf = PDFSampler(num_samples=self.config.num_reflect_importance_samples,
                                              include_original=False)
        self.far = 2**8
        self.near = 1.0 / 16
        # Standard deviation, in scene units, of the opt-in depth term (loss_coefficients["depth_loss_fine" / "depth_loss_coarse"],
        # include/rsn.h: rsn_depth_loss_forward).  A starting point: no scene has been measured.
        self.depth_sigma = 0.1
        self.background_color = torch.tensor([1.0, 1.0, 1.0])  # colors.WHITE
        self.rgb_loss = nn.MSELoss()
        # Checkpoints of the reference: its Model also owns torchmetrics modules (model.py:131-133: psnr, ssim,
        # lpips -- the LPIPS network's weights sit in every pipeline checkpoint as `_model.lpips.net.*`).  This Model has no such
        # modules (SSIM / LPIPS are out of scope), so their entries are dropped from an incoming state dict before nn.Module's strict
        # key check sees them -- also when the checkpoint is loaded through a parent (nerfstudio's pipeline: prefix `_model.`).
        self._register_load_state_dict_pre_hook(self._drop_reference_metric_state)
        self._deterministic = os.environ.get("RSN_DETERMINISTIC", "") == "1"
        self.occupancy = None  # an occupancy.OccupancyGrid: eval renders skip the rays that cross no occupied cell (_cull)
        self.occupancy_samples = False  # with the grid: also evaluate the field only on the samples in occupied cells (_get_outputs_eval)

    _REFERENCE_METRIC_MODULES = ("lpips", "psnr", "ssim")

    @staticmethod
    def _drop_reference_metric_state(state_dict, prefix, *_unused) -> None:
        drop = tuple(prefix + m + "." for m in ReflectSamplingNeRFModel._REFERENCE_METRIC_MODULES)
        for k in [k for k in state_dict if k.startswith(drop)]:
            del state_dict[k]

    @property
    def deterministic(self) -> bool:
        """Bit-reproducible training steps: the weight gradients are reduced in a fixed order (rsn_weight_grad_*_ordered) instead of
        by fp32 atomics.  Default False, or True when the environment holds RSN_DETERMINISTIC=1 as the model is built."""
        return self._deterministic

    def set_deterministic(self, flag: bool) -> None:
        """Same build, device, seed, rays and settings (mma mode, weight_grad_groups, reflect_capacity, ray_chunk) -> the same
        gradient and parameter bits on every run.  Costs one workspace (68 MB at width 256) and a slower reduction flush."""
        self._deterministic = bool(flag)

    def get_param_groups(self) -> Dict[str, List[Parameter]]:
        if self.field is None:
            raise ValueError("populate_fields() must be called before get_param_groups")
        return {"fields": list(self.field.parameters())}

    # ------------------------------------------------------------------ the hot path (model.py:142-344)
    def get_outputs(self, ray_bundle) -> Dict[str, Tensor]:
        if self.field is None:
            raise ValueError("populate_fields() must be called before get_outputs")
        if self.training:
            return self._get_outputs_train(ray_bundle)
        if getattr(self, "occupancy", None) is not None:
            return self._get_outputs_eval_culled(ray_bundle)
        return self._get_outputs_eval(ray_bundle)

    def _get_outputs_train(self, ray_bundle, jitter: Optional[Dict[str, Tensor]] = None,
                           bins: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """Training mode: one autograd node (train_graph.GetOutputsTrain) over the HIP forward/backward kernels.
        `jitter` optionally injects the samplers' uniform draws and `bins` whole sampler outputs
        ({"fine_spacing", "fine_euclid", ...}); tests share them with the oracle / the reference's logged values."""
        from .train_graph import DEPTH_KEYS, DIFF_KEYS, DIST_KEYS, FUSED_KEYS, GetOutputsTrain, depth_levels, distortion_levels

        R = ray_bundle.origins.shape[0]
        o = ops._f32c(ray_bundle.origins.reshape(R, 3))
        d = ops._f32c(ray_bundle.directions.reshape(R, 3))
        pa = ops._f32c(ray_bundle.pixel_area.reshape(R))
        nears = ops._f32c(ray_bundle.nears.reshape(R))
        fars = ops._f32c(ray_bundle.fars.reshape(R))
        # the opt-in depth term's target distances: a constant of the graph, read only when a depth coefficient is set
        meta = getattr(ray_bundle, "metadata", None)
        target = meta.get("depth") if isinstance(meta, dict) else None
        self._depth_target = None if target is None else ops._f32c(target.reshape(-1))
        try:
            outs = GetOutputsTrain.apply(self, o, d, pa, nears, fars, jitter, bins, *self.field.parameters())
        finally:
            self._depth_target = None
        aux = self._train_aux
        self._train_aux = None
        outputs = type(aux)(zip(DIFF_KEYS, outs))  # LazyOutputs: depth_reflect_fine ([M, 1]) on first access
        for k, v in aux.present():  # (not items(): that would materialise the lazy [M, 1] entry -- a host read)
            outputs[k] = v.detach() if v.dtype.is_floating_point else v
        outputs.lazy = aux.lazy
        # not keys of the reference's dict: the normal losses of get_loss_dict, reduced per ray by the compositing kernel
        outputs.fused = dict(zip(FUSED_KEYS, outs[len(DIFF_KEYS):]))
        # opt-in: the per-ray distortion loss of the levels whose coefficient is set (none by default: FUSED_KEYS only)
        on = [k for k, lvl in zip(DIST_KEYS, distortion_levels(self)) if lvl]
        on += [k for k, lvl in zip(DEPTH_KEYS, depth_levels(self)) if lvl]  # and the opt-in depth term's, behind them
        outputs.fused.update(zip(on, outs[len(DIFF_KEYS) + len(FUSED_KEYS):]))
        return outputs

    @property
    def _last_num_reflected(self) -> int:
        """M of the last training-mode get_outputs.  The count lives on the device (`_last_n_masked_dev`): reading it
        here is a device-to-host synchronisation -- diagnostics only, the training step never does."""
        nm = getattr(self, "_last_n_masked_dev", None)
        return 0 if nm is None else int(nm.item())

    @torch.no_grad()
    def _get_outputs_eval(self, ray_bundle, n_dev0: Optional[Tensor] = None, primary_only: bool = False) -> Dict[str, Tensor]:
        """n_dev0 (culled renders only): device int32 count of the bundle's leading rays that are live.  The primary-level launches
        take it as their n_dev; the rows behind it are never computed, and their accumulation is 0 so that rsn_reflect_setup --
        which takes only a host count -- masks none of them.
        primary_only: stop after the two primary levels (steps A and B) and return only what they give (get_surface_outputs)."""
        cfg, fld = self.config, self.field
        R = ray_bundle.origins.shape[0]
        o = ops._f32c(ray_bundle.origins.reshape(R, 3))
        d = ops._f32c(ray_bundle.directions.reshape(R, 3))
        pa = ops._f32c(ray_bundle.pixel_area.reshape(R))
        nears = ops._f32c(ray_bundle.nears.reshape(R))
        fars = ops._f32c(ray_bundle.fars.reshape(R))
        Sc, Sf = cfg.num_coarse_samples, cfg.num_importance_samples
        Src, Srf = cfg.num_reflect_coarse_samples, cfg.num_reflect_importance_samples
        EVAL, CLIP = ops.RSN_COMP_EVAL, ops.RSN_COMP_CLIP_RGB
        uni, rec = self.sampler_uniform.spec, self.sampler_reciprocal.spec
        grid = getattr(self, "occupancy", None) if getattr(self, "occupancy_samples", False) else None

        def evaluate(level_id, *args, **kw):  # the four levels: all samples, or (occupancy_samples) the ones in occupied cells
            if grid is None:
                return fld.evaluate_frustums(*args, **kw)
            return fld.evaluate_frustums_skipping(grid, level_id, *args, **kw)

        # A. coarse primary (model.py:148-177)
        sb_c, eb_c = ops.sample_spaced(R, n_dev0, Sc, uni.spacing, uni.tan, nears, fars, None)
        lc = evaluate(0, o, d, pa, eb_c, n_dev0)
        cc = ops.composite(R, n_dev0, Sc, 1, EVAL | CLIP, lc["sigma"], eb_c, lc["color"])
        # B. fine primary (model.py:182-211) + C. per-ray surface attributes (model.py:215-227)
        sb_f, eb_f = ops.sample_pdf(R, n_dev0, Sc, Sf, uni.spacing, uni.tan, self.sampler_pdf.histogram_padding, nears,
                                    fars, cc["weights"], sb_c, None)
        lf = evaluate(1, o, d, pa, eb_f, n_dev0)
        cf = ops.composite(R, n_dev0, Sf, 1, EVAL | CLIP, lf["sigma"], eb_f, lf["color"], level=lf, surface=True,
                           zero_accumulation=n_dev0 is not None)
        if primary_only:  # the same launches, so the same bits, as the full pass up to here; no reflected ray is set up
            return {"accumulation_coarse": cc["accumulation"].unsqueeze(-1), "accumulation_fine": cf["accumulation"].unsqueeze(-1),
                    "depth_coarse": cc["depth"].unsqueeze(-1), "depth_fine": cf["depth"].unsqueeze(-1)}
        # mask, stable compaction, secondary rays, default reflect colours (model.py:222-229,240-241,267-289)
        rs = ops.reflect_setup(o, d, cf["accumulation"], cf["depth"], cf["normals"], cf["roughness"], float(self.far))
        n_dev = rs["n_masked"]

        outputs = ops.LazyOutputs({
            "mid_rgb_coarse": cc["rgb"],
            "mid_rgb_fine": cf["rgb"],
            "mid_reflect_coarse": rs["reflect_coarse"],
            "mid_reflect_fine": rs["reflect_fine"],
            "accumulation_coarse": cc["accumulation"].unsqueeze(-1),
            "accumulation_fine": cf["accumulation"].unsqueeze(-1),
            "depth_coarse": cc["depth"].unsqueeze(-1),
            "depth_fine": cf["depth"].unsqueeze(-1),
            "weights_coarse": cc["weights"].unsqueeze(-1),
            "weights_fine": cf["weights"].unsqueeze(-1),
            "pred_normals_coarse": lc["pred_normals"],
            "pred_normals_fine": lf["pred_normals"],
            "normals_coarse": lc["pred_normals"],  # eval: normals == predicted normals (model.py:161-162)
            "normals_fine": lf["pred_normals"],
            "n_dot_d_coarse": lc["n_dot_d"].unsqueeze(-1),
            "n_dot_d_fine": lf["n_dot_d"].unsqueeze(-1),
            "diff": cf["diff"],
            "tint": cf["tint"],
            "roughness": cf["roughness"].unsqueeze(-1),
            "mask": rs["mask"].bool(),
        })

        # E-G. reflected rays; every launch below reads M from device memory (no host sync)
        o2, d2, pa2, near2, far2 = rs["origins2"], rs["directions2"], rs["pixel_area2"], rs["nears2"], rs["fars2"]
        bg = fld.evaluate_inf(d2, rs["sqradius"], n_dev)
        sb_rc, eb_rc = ops.sample_spaced(R, n_dev, Src, rec.spacing, rec.tan, near2, far2, None)
        lrc = evaluate(2, o2, d2, pa2, eb_rc, n_dev, full=False)
        crc = ops.composite(R, n_dev, Src, 2, EVAL, lrc["sigma"], eb_rc, lrc["color"], bg_rgb=bg, want_depth=False)
        ops.reflect_combine(R, n_dev, rs["ray_index"], cf["diff"], cf["tint"], crc["rgb"], rs["reflect_coarse"])
        sb_rf, eb_rf = ops.sample_pdf(R, n_dev, Src, Srf, rec.spacing, rec.tan,
                                      self.sampler_reflect_pdf.histogram_padding, near2, far2, crc["weights"], sb_rc,
                                      None)
        lrf = evaluate(3, o2, d2, pa2, eb_rf, n_dev, full=False)
        crf = ops.composite(R, n_dev, Srf, 2, EVAL, lrf["sigma"], eb_rf, lrf["color"], bg_rgb=bg)
        ops.reflect_combine(R, n_dev, rs["ray_index"], cf["diff"], cf["tint"], crf["rgb"], rs["reflect_fine"])

        # depth_reflect_fine is [M, 1] and present only when M > 0 (model.py:341): M stays on the device and the entry is
        # materialised on first use (ops.LazyOutputs) -- get_outputs itself issues no device-to-host read, so a chunked
        # image render enqueues every chunk before anything waits
        outputs.lazy["depth_reflect_fine"] = (n_dev, crf["depth"])
        return outputs

    # ------------------------------------------------------------------ depth-only eval pass (mesh.fuse_depth)
    @torch.no_grad()
    def get_surface_outputs(self, ray_bundle) -> Dict[str, Tensor]:
        """Where the model puts its surface, without the reflections: the coarse and fine primary levels of the eval-mode
        get_outputs and nothing after them -- no reflected rays, no background evaluation, no reflect levels: two of the
        four levels (at the default sample counts 256 of a reflected ray's 384 samples).  -> depth_fine (the median depth the model starts its reflected rays from),
        accumulation_fine, depth_coarse, accumulation_coarse, each [R, 1], with the bits the full pass gives for the same rays.
        The collider fills nears / fars as in forward().  No device-to-host read.  self.occupancy is not consulted: no ray is
        culled here."""
        if self.field is None:
            raise ValueError("populate_fields() must be called before get_surface_outputs")
        if self.collider is not None:
            ray_bundle = self.collider(ray_bundle)
        return self._get_outputs_eval(ray_bundle, primary_only=True)

    @torch.no_grad()
    def get_surface_outputs_for_camera_ray_bundle(self, camera_ray_bundle, chunk: Optional[int] = None) -> Dict[str, Tensor]:
        """get_surface_outputs over a whole image in chunks of `chunk` rays (default: config.eval_num_rays_per_chunk), each key
        reshaped to the image: [H, W, 1].  Every chunk is enqueued on the current stream before anything is read back: no
        device-to-host read per chunk, or at all."""
        chunk = int(self.config.eval_num_rays_per_chunk if chunk is None else chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        image_shape = camera_ray_bundle.origins.shape[:-1]
        n = 1
        for s_ in image_shape:
            n *= int(s_)
        lists: Dict[str, list] = {}
        for i in range(0, n, chunk):
            out = self.get_surface_outputs(camera_ray_bundle.get_row_major_sliced_ray_bundle(i, min(i + chunk, n)))
            for k, v in out.items():
                lists.setdefault(k, []).append(v)
        return {k: torch.cat(v).view(*image_shape, *v[0].shape[1:]) for k, v in lists.items()}

    # ------------------------------------------------------------------ empty-space skipping (occupancy.py)
    def _cull(self, ray_bundle, marks: Optional[list] = None):
        """Cull a flat ray bundle [R] (nears / fars set) against self.occupancy: one rsn_occupancy_cull launch over all R rays and a
        gather of the rays through ray_index -> (the bundle with the hit rays first, the cull's outputs).  The count of hit rays
        stays on the device.

        The eval pipeline then runs on the leading rays only, and rsn_scatter_rows writes every output key back to the rays' own
        rows.  A culled ray holds, per key:

            mid_rgb_coarse, mid_rgb_fine, mid_reflect_coarse, mid_reflect_fine, diff      1 (what compositing zero weights on the
                                                                                           white background gives)
            accumulation_*, tint, roughness, weights_*, pred_normals_*, normals_*, n_dot_d_*   0
            depth_*                                                                        the ray's far
            mask                                                                           false

        A hit ray holds the bits the unculled render gives it: the kernels treat rays independently.  depth_reflect_fine ([M, 1],
        lazy) lists the reflected rays in ascending ray order as before; a culled ray is never among them.

        marks: a list that receives timing events recorded at the start, after the cull and after the gather."""
        from . import occupancy

        R = ray_bundle.origins.shape[0]
        o = ops._f32c(ray_bundle.origins.reshape(R, 3))
        d = ops._f32c(ray_bundle.directions.reshape(R, 3))
        nears = ops._f32c(ray_bundle.nears.reshape(R))
        fars = ops._f32c(ray_bundle.fars.reshape(R))
        ops.record_event(marks)
        culled = occupancy.cull(self.occupancy, o, d, nears, fars)
        culled["fars"] = fars
        ops.record_event(marks)
        compact = ray_bundle[culled["ray_index"].long()]
        ops.record_event(marks)
        return compact, culled

    @torch.no_grad()
    def _get_outputs_eval_culled(self, ray_bundle) -> Dict[str, Tensor]:
        """Eval-mode get_outputs with self.occupancy set: cull, one pass over the compacted rays with the device-side count, scatter."""
        from . import occupancy

        compact_rays, culled = self._cull(ray_bundle)
        compact = self._get_outputs_eval(compact_rays, culled["n_hit"])
        outputs = ops.LazyOutputs(occupancy.scatter_outputs(dict(compact.present()), culled, culled["fars"]))
        outputs.lazy = compact.lazy
        return outputs

    # ------------------------------------------------------------------ eval image, chunked (config.py:41; "next" row §8(f).4)
    @torch.no_grad()
    def get_outputs_for_camera_ray_bundle(self, camera_ray_bundle) -> Dict[str, Tensor]:
        """Chunked full-image rendering: `eval_num_rays_per_chunk` rays per forward (reference config.py:41: 1024),
        per-ray outputs concatenated and reshaped to the image -- what nerfstudio's base Model does, overridden here
        (for nerfstudio's own base class too) so that EVERY CHUNK IS ENQUEUED BEFORE ANYTHING IS READ BACK: get_outputs
        issues no device-to-host read (the one output whose shape needs the reflected-ray count, depth_reflect_fine
        [M, 1], is lazy and is no image anyway; the base class's `.items()` would materialise it once per chunk), so the
        GPU runs chunk after chunk while the host is already launching the following ones.

        With self.occupancy set (occupancy.py) the whole image is culled in one launch, the chunks are cut from the compacted rays,
        chunk i carries the device-side count clamp(n_hit - i * chunk, 0, chunk) into its primary-level launches (the trailing
        chunks run with count 0), and every key is written back with one rsn_scatter_rows; still no device-to-host read.
        While self.occupancy_stage_events is a list, every culled image appends its five timing events to it: start, cull done,
        gather done, chunks done, scatter done (tools/occupancy_report.py)."""
        chunk = self.config.eval_num_rays_per_chunk
        image_shape = camera_ray_bundle.origins.shape[:-1]
        n = 1
        for s_ in image_shape:
            n *= int(s_)
        lists: Dict[str, list] = {}
        n_chunks = 0
        culled = counts = marks = None
        if getattr(self, "occupancy", None) is not None:
            if isinstance(getattr(self, "occupancy_stage_events", None), list):
                marks = []
                self.occupancy_stage_events.append(marks)
            flat = camera_ray_bundle.get_row_major_sliced_ray_bundle(0, n)
            if self.collider is not None:
                flat = self.collider(flat)
            camera_ray_bundle, culled = self._cull(flat, marks)
            starts = torch.arange(0, max(n, 1), chunk, device=culled["n_hit"].device, dtype=torch.int32)
            counts = (culled["n_hit"] - starts).clamp_(0, chunk).to(torch.int32)
        # Small chunks (the reference's 1024 rays) leave the GPU with ramps, tails and a dozen 10-us launches per 3 ms of field
        # kernels: consecutive chunks are independent, so they alternate between two side streams and one chunk's small
        # launches / last partial round of tiles run beside the other's field kernels.
        dev = camera_ray_bundle.origins.device
        side = None
        if dev.type == "cuda" and n > chunk:
            self.field.packed_weights()  # packed once, on the caller's stream, before the side streams read it
            main = torch.cuda.current_stream(dev)
            n_side = int(getattr(self, "eval_side_streams", 3))  # measured: 278 / 310 / 325 / 312 K rays/s with 1 / 2 / 3 / 4 at 1024-ray chunks
            side = getattr(self, "_eval_streams", None)
            if side is None or side[0].device != dev or len(side) != n_side:
                side = self._eval_streams = tuple(torch.cuda.Stream(device=dev) for _ in range(n_side))
            for st in side:
                st.wait_stream(main)
        for i in range(0, n, chunk):
            rb = camera_ray_bundle.get_row_major_sliced_ray_bundle(i, min(i + chunk, n))
            ctx = torch.cuda.stream(side[n_chunks % len(side)]) if side is not None else contextlib.nullcontext()
            n_chunks += 1
            with ctx:
                out = self.forward(rb) if counts is None else self._get_outputs_eval(rb, counts[n_chunks - 1:n_chunks])
            present = out.present() if hasattr(out, "present") else out.items()
            for k, v in present:
                if isinstance(v, Tensor) and v.shape[:1] == (len(rb),):
                    lists.setdefault(k, []).append(v)
        if side is not None:
            for st in side:
                main.wait_stream(st)
            for vs in lists.values():  # allocated on a side stream, read by the caller's stream from here on
                for v in vs:
                    v.record_stream(main)
        # per-ray outputs only: a key that is not [rays, ...] in every chunk (depth_reflect_fine is [M,1]) is no image
        if culled is not None:
            from . import occupancy

            ops.record_event(marks)
            joined: Dict[int, Tensor] = {}  # normals_* are the pred_normals_* tensors: joined and written back once
            compact = {}
            for k, v in lists.items():
                if len(v) == n_chunks and k != "depth_reflect_fine":
                    if id(v[0]) not in joined:
                        joined[id(v[0])] = torch.cat(v)
                    compact[k] = joined[id(v[0])]
            full = occupancy.scatter_outputs(compact, culled, culled["fars"])
            ops.record_event(marks)
            return {k: v.view(*image_shape, *v.shape[1:]) for k, v in full.items()}
        return {k: torch.cat(v).view(*image_shape, *v[0].shape[1:]) for k, v in lists.items()
                if len(v) == n_chunks and k != "depth_reflect_fine"}

    # ------------------------------------------------------------------ loss (model.py:346-430; "next" row §8(f).1)
    def get_loss_dict(self, outputs, batch, metrics_dict=None) -> Dict[str, Tensor]:
        """model.py:346-430: four MSE terms against the (white-blended) image, two predicted-normal and two
        orientation terms, scaled by config.loss_coefficients.  One fused HIP pass (train_ops.FusedLoss).
        Not in the reference, opt-in: distortion_loss_coarse / distortion_loss_fine (mip-NeRF 360 eq. 15) for the levels whose
        coefficient is set and not 0, from the training graph's per-ray terms (train_ops.distortion_loss_dict)."""
        from .train_ops import depth_loss_dict, distortion_loss_dict, fused_loss_dict, fused_ray_loss_dict

        image = batch["image"].to(self.device)
        if image.shape[-1] == 4:  # RGBRenderer.blend_background with the white background colour
            image = image[..., :3] * image[..., 3:] + (1.0 - image[..., 3:])
        fused = getattr(outputs, "fused", None)
        extra = distortion_loss_dict(fused, self.config.loss_coefficients)  # {} by default; raises when set without its fused term
        extra.update(depth_loss_dict(fused, self.config.loss_coefficients))  # likewise: the opt-in depth term
        if fused is not None:  # outputs of this model's own training graph: the per-sample terms are already per-ray sums
            losses = fused_ray_loss_dict(outputs, fused, image, self.config.loss_coefficients)
        else:
            losses = fused_loss_dict(outputs, image, self.config.loss_coefficients)
        losses.update(extra)
        return losses

    # ------------------------------------------------------------------ eval image (model.py:432-482; "next" row §8(f).4)
    def get_image_metrics_and_images(self, outputs: Dict[str, Tensor], batch: Dict[str, Tensor]):
        """Working equivalent of the reference hook (which raises KeyError: 'low_coarse' at model.py:438): PSNR of the
        coarse render and of the reflect-fine render against the white-blended ground truth, and the three panels the
        reference assembles (rgb | accumulation | depth, coarse and fine side by side).  SSIM / LPIPS need the
        torchmetrics networks and are out of scope."""
        assert self.config.collider_params is not None, "mip-NeRF requires collider parameters to be set."
        image = batch["image"].to(outputs["mid_rgb_coarse"].device)
        if image.shape[-1] == 4:
            image = image[..., :3] * image[..., 3:] + (1.0 - image[..., 3:])
        rgb_coarse = torch.clip(outputs["mid_rgb_coarse"], 0.0, 1.0)
        rgb_fine = torch.clip(outputs["mid_reflect_fine"], 0.0, 1.0)

        def psnr(a, b):
            return float(10.0 * torch.log10(1.0 / torch.mean((a - b) ** 2).clamp(min=1e-12)))

        near, far = self.config.collider_params["near_plane"], self.config.collider_params["far_plane"]

        def depth_panel(d, acc):
            return (((d - near) / (far - near)).clamp(0.0, 1.0) * acc + (1.0 - acc)).expand(*d.shape[:-1], 3)

        gray = lambda a: a.expand(*a.shape[:-1], 3)  # noqa: E731
        images = {
            "img": torch.cat([image, rgb_coarse, rgb_fine], dim=1),
            "accumulation": torch.cat([gray(outputs["accumulation_coarse"]), gray(outputs["accumulation_fine"])], dim=1),
            "depth": torch.cat([depth_panel(outputs["depth_coarse"], outputs["accumulation_coarse"]),
                                depth_panel(outputs["depth_fine"], outputs["accumulation_fine"])], dim=1),
        }
        fine_psnr = psnr(image, rgb_fine)
        metrics = {"psnr": fine_psnr, "coarse_psnr": psnr(image, rgb_coarse), "fine_psnr": fine_psnr}
        return metrics, images
