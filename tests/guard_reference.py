"""CPU reference of the guarded optimiser step (numpy / torch): the fp64 sum of squares of a gradient list, the clip coefficient
in fp32 as torch.nn.utils.clip_grad_norm_ forms it, and a RAdam step on g * coef by torch's own clip_grad_norm_ and
torch.optim.RAdam."""
from typing import List, Optional, Sequence

import numpy as np
import torch


def sumsq_fp64(grads: Sequence[Optional[torch.Tensor]]) -> List[float]:
    """Per tensor: sum of (double)g^2 (0.0 for None).  The square of an fp32 value is exact in fp64; the sum's rounding error is at
    most n * 2^-53 relative (all terms are non-negative), whatever the order."""
    out = []
    for g in grads:
        if g is None:
            out.append(0.0)
            continue
        x = g.detach().cpu().numpy().astype(np.float64).ravel()
        out.append(float(np.sum(x * x)))
    return out


def norm_fp32(per_tensor_sq: Sequence[float]) -> np.float32:
    """float32(sqrt(fp64 total)), the tensors summed in index order."""
    total = 0.0
    for s in per_tensor_sq:
        total += s
    return np.float32(np.sqrt(np.float64(total)))


def clip_coef(norm, max_norm: Optional[float]) -> np.float32:
    """clip_grad_norm_'s factor in fp32: clamp(max_norm / (norm + 1e-6), max=1); a NaN stays a NaN.  None / inf / <= 0: 1."""
    if max_norm is None or not np.isfinite(max_norm) or max_norm <= 0.0:
        return np.float32(1.0)
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


def clipped_radam_step(params: Sequence[torch.nn.Parameter], opt: torch.optim.RAdam, max_norm: Optional[float]) -> float:
    """One reference step on the gradients the parameters hold: clip_grad_norm_ (when max_norm is set), then opt.step().
    -> the factor torch applied (1.0 without clipping).  torch rewrites .grad; the caller hands in fresh gradients every step."""
    coef = 1.0
    if max_norm is not None:
        with_grad = [p for p in params if p.grad is not None]
        total = torch.nn.utils.clip_grad_norm_(with_grad, max_norm)
        coef = float(torch.clamp(max_norm / (total + 1e-6), max=1.0))
    opt.step()
    return coef


def skip_radam_step(opt: torch.optim.RAdam) -> None:
    """A skipped iteration under this project's semantics: no parameter and no moment changes, every existing state's step count
    advances by one (the schedule and the bias correction count iterations)."""
    for st in opt.state.values():
        st["step"] += 1
