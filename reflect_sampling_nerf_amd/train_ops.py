"""Loss and optimiser step of the training iteration on the HIP path.

FusedLoss   -- get_loss_dict (reference model.py:346-430) on ANY outputs dict: rsn_loss_forward_backward computes the 8
               terms and their gradients w.r.t. the model outputs in one pass over the samples.
FusedRayLoss-- the same for outputs of this package's training graph: the per-sample normal terms were already reduced
               per ray in the compositing epilogue, the loss is two launches over R rays.
FusedRAdam  -- torch.optim.RAdam semantics (reference config.py:50-53) as one multi-tensor launch (rsn_radam_step),
               with the reference's exponential learning-rate decay (lr 1e-3 -> 1e-4 over 50 000 steps).  Opt-in guard:
               global gradient-norm clipping and the skip of a step with non-finite gradients, two launches
               (rsn_grad_sumsq, rsn_radam_step_guarded), still without a host read.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Sequence

import torch
from torch import Tensor

from . import _abi, ops
from ._abi import check, ptr

LOSS_TERMS = ("loss_mid_coarse", "loss_mid_fine", "loss_reflect_mid_coarse", "loss_reflect_mid_fine",
              "predicted_normal_loss_coarse", "predicted_normal_loss_fine", "orientation_loss_coarse",
              "orientation_loss_fine")


def _ptr_array(tensors: List[Optional[Tensor]]):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


class FusedLoss(torch.autograd.Function):
    """(image, coef[8], rgb x4, weights x2, normals x2, pred_normals x2, n_dot_d x2) -> scaled losses [8]."""

    @staticmethod
    def forward(ctx, image, coef, rgb_c, rgb_f, refl_c, refl_f, w_c, w_f, n_c, n_f, pn_c, pn_f, ndd_c, ndd_f):
        lib = _abi.load_library()
        f = ops._f32c
        image = f(image)
        rgb = [f(rgb_c), f(rgb_f), f(refl_c), f(refl_f)]
        R = rgb[0].shape[0]
        w = [f(w_c.reshape(R, -1)), f(w_f.reshape(R, -1))]
        Sc, Sf = w[0].shape[1], w[1].shape[1]
        nrm = [f(n_c.reshape(R, Sc, 3)), f(n_f.reshape(R, Sf, 3))]
        pn = [f(pn_c.reshape(R, Sc, 3)), f(pn_f.reshape(R, Sf, 3))]
        ndd = [f(ndd_c.reshape(R, Sc)), f(ndd_f.reshape(R, Sf))]
        dev = image.device
        losses = torch.empty(8, device=dev)
        g_rgb = [torch.empty_like(t) for t in rgb]
        g_pn = [torch.empty_like(t) for t in pn]
        g_ndd = [torch.empty_like(t) for t in ndd]
        coef_arr = (C.c_float * 8)(*[float(c) for c in coef])
        check(lib.rsn_loss_forward_backward(R, Sc, Sf, ptr(image), _ptr_array(rgb), _ptr_array(w), _ptr_array(nrm),
                                            _ptr_array(pn), _ptr_array(ndd), coef_arr, ptr(losses), _ptr_array(g_rgb),
                                            _ptr_array(g_pn), _ptr_array(g_ndd), ops._stream()))
        ctx.grads = (g_rgb, g_pn, g_ndd)
        ctx.dims = (R, Sc, Sf)
        ctx.shapes = (pn_c.shape, pn_f.shape, ndd_c.shape, ndd_f.shape)
        key = (tuple(float(c) for c in coef), dev)
        if FusedLoss._coef_cache[0] != key:  # the coefficients change twice per run (warm-up): no per-step upload
            FusedLoss._coef_cache = (key, torch.tensor([float(c) for c in coef], device=dev))
        return losses * FusedLoss._coef_cache[1]

    _coef_cache = (None, None)

    @staticmethod
    def backward(ctx, g8):
        lib = _abi.load_library()
        if ctx.grads is None:
            raise RuntimeError("FusedLoss: the gradient buffers are scaled in place; backward can run once per forward")
        g_rgb, g_pn, g_ndd = ctx.grads
        ctx.grads = None
        R, Sc, Sf = ctx.dims
        s = ctx.shapes
        # chain rule with the upstream gradients of the eight terms, in place, one launch (they stay on the device)
        check(lib.rsn_loss_scale_grads(R, Sc, Sf, ptr(ops._f32c(g8)), _ptr_array(g_rgb), _ptr_array(g_pn),
                                       _ptr_array(g_ndd), ops._stream()))
        out = [None, None]
        out += list(g_rgb)
        out += [None, None, None, None]  # weights, normals: constants of the loss (detached in the reference)
        out += [g_pn[0].reshape(s[0]), g_pn[1].reshape(s[1]), g_ndd[0].reshape(s[2]), g_ndd[1].reshape(s[3])]
        return tuple(out)


def fused_loss_dict(outputs: Dict[str, Tensor], image: Tensor, coefficients: Dict[str, float]) -> Dict[str, Tensor]:
    coef = [float(coefficients.get(k, 1.0)) for k in LOSS_TERMS]
    scaled = FusedLoss.apply(image, coef, outputs["mid_rgb_coarse"], outputs["mid_rgb_fine"],
                             outputs["mid_reflect_coarse"], outputs["mid_reflect_fine"], outputs["weights_coarse"],
                             outputs["weights_fine"], outputs["normals_coarse"], outputs["normals_fine"],
                             outputs["pred_normals_coarse"], outputs["pred_normals_fine"], outputs["n_dot_d_coarse"],
                             outputs["n_dot_d_fine"])
    return dict(zip(LOSS_TERMS, scaled.unbind(0)))  # one backward node (a stack) instead of eight select_backwards


class FusedRayLoss(torch.autograd.Function):
    """(image, coef[8], rgb x4 [R,3], pn_loss_ray x2 [R], ori_loss_ray x2 [R]) -> scaled losses [8].

    The training graph reduces the two per-sample normal terms of get_loss_dict (model.py:403-407) per ray inside the
    compositing kernel, where the weights are in registers (train_graph.FUSED_KEYS); what is left of the loss is work on
    R rays: one launch forward (rsn_loss_rays_forward), one backward.  The per-sample gradients d/d pred_normals,
    d/d n_dot_d are formed inside the field's backward kernel from the per-ray upstream gradients returned here."""

    @staticmethod
    def forward(ctx, image, coef, rgb_c, rgb_f, refl_c, refl_f, pnr_c, pnr_f, orr_c, orr_f):
        lib = _abi.load_library()
        f = ops._f32c
        image = f(image)
        rgb = [f(rgb_c), f(rgb_f), f(refl_c), f(refl_f)]
        R = rgb[0].shape[0]
        pnr, orr = [f(pnr_c), f(pnr_f)], [f(orr_c), f(orr_f)]
        dev = image.device
        losses = torch.empty(8, device=dev)
        g_rgb = [torch.empty_like(t) for t in rgb]
        coef_arr = (C.c_float * 8)(*[float(c) for c in coef])
        check(lib.rsn_loss_rays_forward(R, ptr(image), _ptr_array(rgb), _ptr_array(pnr), _ptr_array(orr), coef_arr,
                                        ptr(losses), _ptr_array(g_rgb), ops._stream()))
        ctx.g_rgb, ctx.R, ctx.coef_arr = g_rgb, R, coef_arr
        key = (tuple(float(c) for c in coef), dev)
        if FusedLoss._coef_cache[0] != key:  # the coefficients change twice per run (warm-up): no per-step upload
            FusedLoss._coef_cache = (key, torch.tensor([float(c) for c in coef], device=dev))
        return losses * FusedLoss._coef_cache[1]

    @staticmethod
    def backward(ctx, g8):
        lib = _abi.load_library()
        if ctx.g_rgb is None:
            raise RuntimeError("FusedRayLoss: the gradient buffers are scaled in place; backward can run once per forward")
        g_rgb, R = ctx.g_rgb, ctx.R
        ctx.g_rgb = None
        dev = g_rgb[0].device
        g_pn = [torch.empty(R, device=dev), torch.empty(R, device=dev)]
        g_or = [torch.empty(R, device=dev), torch.empty(R, device=dev)]
        check(lib.rsn_loss_rays_backward(R, ptr(ops._f32c(g8)), ctx.coef_arr, _ptr_array(g_rgb), _ptr_array(g_pn),
                                         _ptr_array(g_or), ops._stream()))
        return (None, None, *g_rgb, *g_pn, *g_or)


def fused_ray_loss_dict(outputs: Dict[str, Tensor], fused: Dict[str, Tensor], image: Tensor,
                        coefficients: Dict[str, float]) -> Dict[str, Tensor]:
    coef = [float(coefficients.get(k, 1.0)) for k in LOSS_TERMS]
    scaled = FusedRayLoss.apply(image, coef, outputs["mid_rgb_coarse"], outputs["mid_rgb_fine"],
                                outputs["mid_reflect_coarse"], outputs["mid_reflect_fine"], fused["pn_loss_ray_coarse"],
                                fused["pn_loss_ray_fine"], fused["ori_loss_ray_coarse"], fused["ori_loss_ray_fine"])
    return dict(zip(LOSS_TERMS, scaled.unbind(0)))


# loss-coefficient key -> the training graph's per-ray output it scales (train_graph.DIST_COEF_KEYS / DIST_KEYS)
DISTORTION_TERMS = (("distortion_loss_coarse", "dist_loss_ray_coarse"), ("distortion_loss_fine", "dist_loss_ray_fine"))


def distortion_loss_dict(fused: Optional[Dict[str, Tensor]], coefficients: Dict[str, float]) -> Dict[str, Tensor]:
    """The opt-in distortion terms of get_loss_dict: coef * mean over the rays of the level's per-ray loss (nerfstudio's
    distortion_loss takes the same mean), for every level whose coefficient is present and not 0.  Device tensors: the mean is one
    torch reduction over R floats, nothing is read back.  A coefficient that is set on outputs without the level's fused term
    (outputs that did not come from this package's training graph) is an error: the term is never dropped silently."""
    out = {}
    for key, ray_key in DISTORTION_TERMS:
        coef = float(coefficients.get(key, 0.0))
        if coef == 0.0:
            continue
        if fused is None or ray_key not in fused:
            raise _abi.RsnError(f"loss_coefficients[{key!r}] = {coef:g}, but the outputs carry no fused {ray_key!r}: the distortion loss "
                                "exists only on the outputs of this model's own training graph (model.train(); get_outputs)")
        out[key] = coef * fused[ray_key].mean()
    return out


# likewise for the opt-in depth term (train_graph.DEPTH_COEF_KEYS / DEPTH_KEYS)
DEPTH_TERMS = (("depth_loss_coarse", "depth_loss_ray_coarse"), ("depth_loss_fine", "depth_loss_ray_fine"))


def depth_loss_dict(fused: Optional[Dict[str, Tensor]], coefficients: Dict[str, float]) -> Dict[str, Tensor]:
    """The opt-in DS-NeRF depth terms of get_loss_dict: coef * mean over ALL the rays of the level's per-ray loss (a ray without a
    target contributes 0 to the sum and counts in the mean, as in nerfstudio's depth loss), for every level whose coefficient is
    present and not 0.  Device tensors, nothing is read back.  A coefficient that is set on outputs without the level's fused term
    is an error: the term is never dropped silently."""
    out = {}
    for key, ray_key in DEPTH_TERMS:
        coef = float(coefficients.get(key, 0.0))
        if coef == 0.0:
            continue
        if fused is None or ray_key not in fused:
            raise _abi.RsnError(f"loss_coefficients[{key!r}] = {coef:g}, but the outputs carry no fused {ray_key!r}: the depth loss "
                                "exists only on the outputs of this model's own training graph (model.train(); get_outputs) for rays "
                                "that carry a target (ray_bundle.metadata['depth'])")
        out[key] = coef * fused[ray_key].mean()
    return out


def exponential_decay_lr(step: int, lr_init: float = 1e-3, lr_final: float = 1e-4, max_steps: int = 50000) -> float:
    """nerfstudio ExponentialDecayScheduler without warm-up (reference config.py:52): log-linear interpolation."""
    t = min(max(step / max_steps, 0.0), 1.0)
    return float(lr_init * (lr_final / lr_init) ** t)


# rsn_grad_sumsq's grid (csrc/rsn_train_ops.hip: GUARD_THREADS, GUARD_VEC, GUARD_SLOTS; test_guard_cpu compares): a tensor of more
# than GUARD_SLOTS * GUARD_THREADS * GUARD_VEC elements is walked by a grid-stride loop
GUARD_THREADS, GUARD_VEC, GUARD_SLOTS = 256, 4, 8


class FusedRAdam:
    """RAdam (torch.optim.RAdam semantics, weight_decay 0) over a fixed parameter list, one kernel launch per step.

    The guard (both parts off by default; with both off step() is the one launch above):
      max_grad_norm   -- clip the global L2 norm of all gradients to this value before the update, as
                         torch.nn.utils.clip_grad_norm_ does (nerfstudio's OptimizerConfig.max_norm); None or inf: no clipping.
                         The update reads g * coef; .grad itself is not rewritten (torch rewrites it).
      skip_nonfinite  -- a step whose gradients hold an inf or a NaN changes no parameter and no moment (what torch's
                         GradScaler.step does for the reference under mixed_precision=True).
    With either on, step() is two launches, rsn_grad_sumsq and rsn_radam_step_guarded, and still reads nothing back: the
    decision is taken on the device.  guard_stats() is the explicit read.

    A skipped step still advances step_count, hence the learning-rate schedule and the bias-correction `t`: both count
    iterations.  torch's scaler does not advance `t` on a skipped step; the difference is one step of bias correction per
    skip.  In exchange there is no device-side counter, no host read, and no optimiser state beyond torch.optim.RAdam's:
    state_dict() is the same with and without the guard, and so is a bit-exact resume.

    names: optional parameter names, in the order of `params` (all of them, before the requires_grad filter); guard_stats()
    keys its per-parameter entries by them."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-15,
                 lr_final: Optional[float] = None, max_steps: int = 50000, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, names: Optional[Sequence[str]] = None):
        params = list(params)
        if names is not None and len(names) != len(params):
            raise ValueError(f"{len(names)} names for {len(params)} parameters")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:  # a NaN fails this too
            raise ValueError(f"max_grad_norm must be above 0 (None: no clipping), got {max_grad_norm!r}")
        self.names: Optional[List[str]] = None if names is None else [str(n) for n, p in zip(names, params) if p.requires_grad]
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard_ws: Optional[Tensor] = None     # rsn_grad_sumsq's partial sums; allocated by the first guarded step
        self._guard_stats: Optional[Tensor] = None  # one rsn_guard_stats, as int32 words
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        self.lr, self.betas, self.eps = lr, betas, eps
        self.lr_final, self.max_steps = lr_final, max_steps
        self.step_count = 0
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self._sizes = (C.c_int32 * len(self.params))(*[p.numel() for p in self.params])

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    # -- checkpoint / resume in torch.optim.RAdam's own format: a run of the reference (nerfstudio's RAdamOptimizerConfig builds
    #    torch.optim.RAdam; its trainer saves optimizer.state_dict()) resumes here and the other way round.
    def state_dict(self) -> dict:
        state = {}
        for i, (m, v) in enumerate(zip(self.exp_avg, self.exp_avg_sq)):
            if self.step_count > 0:
                state[i] = {"step": torch.tensor(float(self.step_count)), "exp_avg": m, "exp_avg_sq": v}
        group = {"lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": 0, "decoupled_weight_decay": False,
                 "foreach": None, "maximize": False, "capturable": False, "differentiable": False,
                 "params": list(range(len(self.params)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd: dict) -> None:
        """Everything is checked before anything is changed: a rejected state dict leaves the optimiser as it was.
        The learning rate: without a schedule (lr_final None) `lr` of the first group, as torch.  With one, self.lr is the BASE rate
        that current_lr() decays from step_count, and a torch optimiser under a scheduler (the reference: LambdaLR) keeps its
        already-decayed rate in `lr` and the base rate in `initial_lr`: that one is taken when present, else self.lr stays as
        constructed (this class's own state dicts carry the base rate in `lr` and no `initial_lr`)."""
        groups = sd["param_groups"]
        ids = [i for g in groups for i in g["params"]]
        if len(ids) != len(self.params):
            raise ValueError(f"optimizer state for {len(ids)} parameters, this optimizer has {len(self.params)}")
        g0 = groups[0]
        if any(g.get("weight_decay", 0) != 0 for g in groups):
            raise ValueError("FusedRAdam has no weight decay (the reference trains without: config.py:50-53)")
        if self.lr_final is None:
            lr = float(g0["lr"])
        else:
            lr = float(g0["initial_lr"]) if g0.get("initial_lr") is not None else self.lr
        betas, eps = tuple(g0["betas"]), float(g0["eps"])
        steps, moments = set(), []
        for k, pid in enumerate(ids):  # k-th parameter of this optimizer <- state entry `pid` (torch numbers them in group order)
            st = sd["state"].get(pid)
            p = self.params[k]
            if st is None:  # torch creates a parameter's state at its first gradient: none yet = zeros
                moments.append(None)
                continue
            for name in ("exp_avg", "exp_avg_sq"):
                if tuple(st[name].shape) != tuple(p.shape):
                    raise ValueError(f"parameter {k}: {name} of shape {tuple(st[name].shape)}, parameter {tuple(p.shape)}")
            moments.append((st["exp_avg"], st["exp_avg_sq"]))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"per-parameter step counts differ ({sorted(steps)}): the fused kernel keeps one step count")
        self.lr, self.betas, self.eps = lr, betas, eps
        for k, (mv, p) in enumerate(zip(moments, self.params)):
            if mv is None:
                self.exp_avg[k].zero_()
                self.exp_avg_sq[k].zero_()
            else:
                self.exp_avg[k] = mv[0].detach().to(device=p.device, dtype=p.dtype).clone()
                self.exp_avg_sq[k] = mv[1].detach().to(device=p.device, dtype=p.dtype).clone()
        self.step_count = steps.pop() if steps else 0

    def current_lr(self) -> float:
        if self.lr_final is None:
            return self.lr
        return exponential_decay_lr(self.step_count, self.lr, self.lr_final, self.max_steps)

    @property
    def guarded(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _guarded_launches(self, lib, grads, lr: float) -> None:
        n, dev = len(self.params), self.params[0].device
        if self._guard_ws is None or self._guard_ws.device != dev:
            nbytes = lib.rsn_grad_sumsq_workspace_bytes(n, self._sizes)
            if nbytes == 0:
                check(-1)  # raises with the message rsn_last_error() holds
            self._guard_ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)  # written before it is read, every call
            self._guard_stats = torch.zeros(C.sizeof(_abi.GuardStats) // 4, dtype=torch.int32, device=dev)
        ws, ws_bytes = ptr(self._guard_ws), self._guard_ws.numel() * 8
        g = _ptr_array(grads)
        check(lib.rsn_grad_sumsq(n, g, self._sizes, ws, ws_bytes, ops._stream()))
        max_norm = 0.0 if self.max_grad_norm is None or math.isinf(self.max_grad_norm) else self.max_grad_norm
        check(lib.rsn_radam_step_guarded(n, _ptr_array([p.data for p in self.params]), g, _ptr_array(self.exp_avg),
                                         _ptr_array(self.exp_avg_sq), self._sizes, self.step_count, lr, self.betas[0],
                                         self.betas[1], self.eps, max_norm, int(self.skip_nonfinite), ws, ws_bytes,
                                         ptr(self._guard_stats), ops._stream()))

    def guard_stats(self) -> Optional[dict]:
        """What the last guarded step recorded on the device, by ONE explicit device-to-host read (step() never calls this):
        last_norm (the global gradient norm), last_coef (the factor the gradients were read with), last_skipped (that step),
        skipped_total, last_skipped_step (the step_count of the last skipped step, None: none so far), per_tensor_sq and
        per_tensor_sq_at_last_skip (sum of squares per parameter of the last step / of the last skipped step, keyed by
        `names`, else by index) and nonfinite_at_last_skip (the keys whose sum was not finite then).  None before the
        first guarded step."""
        if self._guard_stats is None:
            return None
        st = _abi.GuardStats.from_buffer_copy(self._guard_stats.cpu().numpy().tobytes())
        keys = self.names if self.names is not None else list(range(len(self.params)))
        at_skip = {k: float(st.per_tensor_sq_at_last_skip[i]) for i, k in enumerate(keys)}
        return {"last_norm": float(st.last_norm), "last_coef": float(st.last_coef), "last_skipped": bool(st.last_skipped),
                "skipped_total": int(st.skipped_total),
                "last_skipped_step": int(st.last_skipped_step) if st.last_skipped_step > 0 else None,
                "per_tensor_sq": {k: float(st.per_tensor_sq[i]) for i, k in enumerate(keys)},
                "per_tensor_sq_at_last_skip": at_skip,
                "nonfinite_at_last_skip": [k for k, v in at_skip.items() if not math.isfinite(v)] if st.skipped_total > 0 else []}

    @torch.no_grad()
    def step(self) -> None:
        lib = _abi.load_library()
        lr = self.current_lr()
        self.step_count += 1
        if self.exp_avg[0].device != self.params[0].device:  # parameters were moved after construction
            self.exp_avg = [m.to(p.device) for m, p in zip(self.exp_avg, self.params)]
            self.exp_avg_sq = [v.to(p.device) for v, p in zip(self.exp_avg_sq, self.params)]
        grads = [None if p.grad is None else ops._f32c(p.grad) for p in self.params]
        if not self.guarded:
            check(lib.rsn_radam_step(len(self.params), _ptr_array([p.data for p in self.params]), _ptr_array(grads),
                                     _ptr_array(self.exp_avg), _ptr_array(self.exp_avg_sq), self._sizes, self.step_count,
                                     lr, self.betas[0], self.betas[1], self.eps, ops._stream()))
        else:
            self._guarded_launches(lib, grads, lr)
        # The kernel updated the parameters behind torch's back: bump their version counters so that consumers keyed on
        # Tensor._version (the Field's packed-weights cache) see the change.
        touched = [p for p in self.params if p.grad is not None]
        setter = getattr(torch._C._autograd, "_unsafe_set_version_counter", None)
        if setter is not None:
            setter(touched, [p._version + 1 for p in touched])
        else:  # pragma: no cover - older torch: a no-op in-place op bumps the counter
            for p in touched:
                p.data.mul_(1.0)
