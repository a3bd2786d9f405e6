"""Image metrics of the reference's evaluation (reflect_sampling_nerf_model.py:468-479), computed on the device.

Both functions take [H,W,3] fp32 images (pred, target) and return a 0-d tensor on their device without reading anything
back.  `ssim` is torchmetrics' structural_similarity_index_measure with the defaults the reference uses (model.py:131,470),
fused into one HIP tile kernel plus a fixed-order reduction (rsn_ssim, include/rsn.h).  LPIPS needs pretrained network
weights this package does not ship and is not provided.
"""
from __future__ import annotations

import torch

from . import _abi


def _check_images(pred: torch.Tensor, target: torch.Tensor):
    if pred.dim() != 3 or pred.shape[-1] != 3 or pred.shape != target.shape:
        raise ValueError(f"expected two [H,W,3] images, got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.device != target.device:
        raise ValueError(f"images on {pred.device} and {target.device}")


def psnr(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """10 log10(1 / mse), data range 1 (torchmetrics PeakSignalNoiseRatio(data_range=1.0), model.py:130)."""
    _check_images(pred, target)
    mse = torch.mean((pred.float() - target.float()) ** 2)
    return 10.0 * torch.log10(1.0 / mse)


def ssim(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Mean SSIM over the channels and the (H-10) x (W-10) full-window positions; images of at least 11 x 11."""
    _check_images(pred, target)
    if pred.device.type != "cuda":
        raise ValueError(f"ssim runs on the GPU (rsn_ssim); got images on {pred.device}")
    H, W = int(pred.shape[0]), int(pred.shape[1])
    lib = _abi.load_library()
    p = pred.float().contiguous()
    t = target.float().contiguous()
    pmin, pmax = torch.aminmax(p)
    tmin, tmax = torch.aminmax(t)
    data_range = torch.maximum(pmax - pmin, tmax - tmin)
    nbytes = int(lib.rsn_ssim_workspace_bytes(H, W))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=p.device)
    out = torch.empty((), dtype=torch.float32, device=p.device)
    stream = torch.cuda.current_stream(p.device).cuda_stream
    _abi.check(lib.rsn_ssim(H, W, _abi.ptr(p), _abi.ptr(t), _abi.ptr(data_range), _abi.ptr(ws), nbytes, _abi.ptr(out),
                            stream))
    return out
