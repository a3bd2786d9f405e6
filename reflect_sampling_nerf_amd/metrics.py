"""Image metrics of the reference's evaluation (reflect_sampling_nerf_model.py:468-479), computed on the device.

`psnr` and `ssim` take [H,W,3] fp32 images (pred, target) and return a 0-d tensor on their device without reading anything
back.  `ssim` is torchmetrics' structural_similarity_index_measure with the defaults the reference uses (model.py:131,470),
fused into one HIP tile kernel plus a fixed-order reduction (rsn_ssim, include/rsn.h).  LPIPS needs pretrained network
weights this package does not ship and is not provided.  `normal_error` is the geometry side of the Ref-NeRF family's tables: the
alpha-weighted mean angular error of a view's composited predicted normals against a ground-truth normal map (rsn_normal_error).
"""
from __future__ import annotations

from typing import Dict, Optional

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


def normal_error(normals: torch.Tensor, accumulation: Optional[torch.Tensor], gt_normals: torch.Tensor, gt_rgba: torch.Tensor,
                 c2w: Optional[torch.Tensor] = None, error_map: bool = False) -> Dict[str, torch.Tensor]:
    """A view's composited predicted normals against its ground-truth normal map (rsn_normal_error, include/rsn.h): the alpha-weighted
    mean angular error in degrees of multinerf's compute_normal_mae, and the accumulation's mean absolute error against the alpha.

    normals fp32 [H,W,3], of any length per pixel (the angle does not depend on it); accumulation fp32 [H,W,1] or [H,W], or None;
    gt_normals uint8 [H,W,3], the bytes of the normal map (n * 0.5 + 0.5); gt_rgba uint8 [H,W,4], or float RGBA in [0, 1] as
    RayDataManager.image returns it (its alpha goes back to its byte, rint(a * 255), on the device).  A pixel counts when its alpha is
    above zero and its normal bytes are not all 127 or 128 (the background of a normal map).  c2w [3,4] or [4,4] on the device: the
    maps are in that camera's frame (OpenGL axes, as the poses use them) and are rotated into the world by c2w[:3,:3] first.

    -> 0-d tensors on the device: normal_mae (NaN when no pixel counts), normal_weight (the summed alpha / 255 of the pixels that
    count), alpha_mae (0 without an accumulation), normal_pixels; with error_map=True also error_map fp32 [H,W], degrees, 0 where the
    pixel does not count.  Two launches, no device-to-host read."""
    if normals.dim() != 3 or normals.shape[-1] != 3 or normals.dtype != torch.float32:
        raise ValueError(f"normals must be float32 [H,W,3], got {normals.dtype} {tuple(normals.shape)}")
    H, W = int(normals.shape[0]), int(normals.shape[1])
    dev = normals.device
    if dev.type != "cuda":
        raise ValueError(f"normal_error runs on the GPU (rsn_normal_error); got normals on {dev}")
    if gt_normals.dtype != torch.uint8 or tuple(gt_normals.shape) != (H, W, 3):
        raise ValueError(f"gt_normals must be uint8 [{H},{W},3], got {gt_normals.dtype} {tuple(gt_normals.shape)}")
    if tuple(gt_rgba.shape) != (H, W, 4) or not (gt_rgba.dtype == torch.uint8 or gt_rgba.is_floating_point()):
        raise ValueError(f"gt_rgba must be uint8 or float [{H},{W},4], got {gt_rgba.dtype} {tuple(gt_rgba.shape)}")
    if accumulation is not None and (accumulation.dtype != torch.float32 or tuple(accumulation.shape) not in ((H, W), (H, W, 1))):
        raise ValueError(f"accumulation must be float32 [{H},{W}] or [{H},{W},1], got {accumulation.dtype} {tuple(accumulation.shape)}")
    if c2w is not None and (c2w.dim() != 2 or tuple(c2w.shape) not in ((3, 4), (4, 4))):
        raise ValueError(f"c2w must be [3,4] or [4,4], got {tuple(c2w.shape)}")
    for name, t in (("accumulation", accumulation), ("gt_normals", gt_normals), ("gt_rgba", gt_rgba), ("c2w", c2w)):
        if t is not None and t.device != dev:
            raise ValueError(f"normals on {dev} and {name} on {t.device}")
    if H * W < 1 or H * W > _abi.RSN_NORMAL_ERROR_MAX_PIXELS:
        raise ValueError(f"{H} x {W} pixels: need 1 to 2^24")
    lib = _abi.load_library()
    if gt_rgba.dtype != torch.uint8:
        alpha = torch.clamp(torch.round(gt_rgba[..., 3].float() * 255.0), 0.0, 255.0).to(torch.uint8)  # round: half to even, rint
        gt_rgba = torch.zeros(H, W, 4, dtype=torch.uint8, device=dev)  # only the alpha byte is read
        gt_rgba[..., 3] = alpha
    n, g, a = normals.contiguous(), gt_normals.contiguous(), gt_rgba.contiguous()
    acc = None if accumulation is None else accumulation.contiguous()
    rot = None if c2w is None else c2w[:3, :3].to(torch.float32).contiguous()
    emap = torch.empty(H, W, dtype=torch.float32, device=dev) if error_map else None
    nbytes = int(lib.rsn_normal_error_workspace_bytes(H * W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    _abi.check(lib.rsn_normal_error(H * W, _abi.ptr(n), _abi.ptr(acc), _abi.ptr(g), _abi.ptr(a), _abi.ptr(rot), _abi.ptr(emap),
                                    _abi.ptr(ws), nbytes, _abi.ptr(out), torch.cuda.current_stream(dev).cuda_stream))
    res = {"normal_mae": out[0], "normal_weight": out[1], "alpha_mae": out[2], "normal_pixels": out[3]}
    if error_map:
        res["error_map"] = emap
    return res


def depth_error(depth: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """A view's rendered depth against its target distances along the rays (rsn_depth_error, include/rsn.h).

    depth fp32 [H,W] or [H,W,1] (outputs["depth_fine"]); target fp32 [H,W] or [H*W], what ops.gather_ray_depth gives for every pixel
    of the view, 0 = no measurement; mask uint8 or bool [H,W] or None, a capture's mask of the view: 0 = the pixel is not scored.

    -> 0-d tensors on the device: depth_mae and depth_rmse over the scored pixels (NaN when there is none), depth_pixels, their
    number, and depth_valid, their share of the view; depth_sums fp32 [3], the kernel's (sum |e|, sum e^2, count).  Two launches, no
    device-to-host read."""
    if depth.dtype != torch.float32 or depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.shape[-1] != 1):
        raise ValueError(f"depth must be float32 [H,W] or [H,W,1], got {depth.dtype} {tuple(depth.shape)}")
    H, W = int(depth.shape[0]), int(depth.shape[1])
    dev = depth.device
    if dev.type != "cuda":
        raise ValueError(f"depth_error runs on the GPU (rsn_depth_error); got depth on {dev}")
    if target.dtype != torch.float32 or target.numel() != H * W:
        raise ValueError(f"target must be float32 with {H} x {W} entries, got {target.dtype} {tuple(target.shape)}")
    if mask is not None and (mask.dtype not in (torch.uint8, torch.bool) or mask.numel() != H * W):
        raise ValueError(f"mask must be uint8 or bool with {H} x {W} entries, got {mask.dtype} {tuple(mask.shape)}")
    for name, t in (("target", target), ("mask", mask)):
        if t is not None and t.device != dev:
            raise ValueError(f"depth on {dev} and {name} on {t.device}")
    if H * W < 1 or H * W > _abi.RSN_NORMAL_ERROR_MAX_PIXELS:
        raise ValueError(f"{H} x {W} pixels: need 1 to 2^24")
    lib = _abi.load_library()
    d, t = depth.contiguous(), target.contiguous()
    m = None if mask is None else mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()
    nbytes = int(lib.rsn_normal_error_workspace_bytes(H * W))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(3, dtype=torch.float32, device=dev)
    _abi.check(lib.rsn_depth_error(H * W, _abi.ptr(d), _abi.ptr(t), _abi.ptr(m), _abi.ptr(ws), nbytes, _abi.ptr(out),
                                   torch.cuda.current_stream(dev).cuda_stream))
    return {"depth_mae": out[0] / out[2], "depth_rmse": torch.sqrt(out[1] / out[2]), "depth_pixels": out[2],
            "depth_valid": out[2] / float(H * W), "depth_sums": out}
