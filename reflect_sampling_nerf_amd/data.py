"""Posed image sets without nerfstudio: a Blender-format parser and a device-resident ray data manager.

`load_blender_split` follows nerfstudio 0.3's BlenderDataParser (the reference trains with it: reflect_sampling_nerf_config.py:36-41);
`RayDataManager.next_train` is the reference datamanager's next_train (reflect_sampling_nerf_datamanager.py:49-58: pixel sampler ->
pixel gather -> ray generator) as ONE launch of rsn_sample_camera_rays on the images uploaded once: no host work beyond the launch,
no device-to-host read.  The exact sampling and ray recipes are in include/rsn.h.

`RayDataManager(..., levels=L)` with L > 1 is mip-NeRF's multi-scale protocol: rsn_build_pyramid forms every image at 1/2 .. 1/2^(L-1)
of its size once, next_train draws each ray's level with probability 1/L (rsn_sample_pyramid_rays, still one launch), and
camera_ray_bundle / image take a level.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _abi
from .nerfstudio_compat import RayBundle


@dataclass
class BlenderScene:
    """One split of a posed image set: images uint8 [N,H,W,4] RGBA (alpha 255 for RGB sources), c2w float32 [N,3,4],
    one pinhole camera (fx, fy, cx, cy) shared by all images.  normals: None, or the ground-truth normal maps uint8 [N,H,W,3], the
    bytes of the scene's normal images, encoding n * 0.5 + 0.5 (eval's geometry metrics read them; training never does)."""

    images: np.ndarray
    c2w: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float
    normals: Optional[np.ndarray] = None

    @property
    def num_images(self) -> int:
        return int(self.images.shape[0])

    @property
    def height(self) -> int:
        return int(self.images.shape[1])

    @property
    def width(self) -> int:
        return int(self.images.shape[2])

    @classmethod
    def from_arrays(cls, images, c2w, focal: float, cx=None, cy=None, normals=None) -> "BlenderScene":
        """images [N,H,W,3|4] (uint8, or float in [0, 1] rounded to uint8), c2w [N,3,4] or [N,4,4]; fx = fy = focal,
        principal point at the image centre unless given.  normals: None, or [N,H,W,3] normal maps -- uint8 taken as is, float unit
        vectors encoded as rint((n * 0.5 + 0.5) * 255) clipped to 0..255."""
        im = np.asarray(images.cpu() if isinstance(images, torch.Tensor) else images)
        if im.ndim != 4 or im.shape[-1] not in (3, 4):
            raise ValueError(f"images must be [N,H,W,3|4], got {im.shape}")
        if im.dtype != np.uint8:
            im = np.clip(np.rint(im.astype(np.float64) * 255.0), 0, 255).astype(np.uint8)
        if im.shape[-1] == 3:
            im = np.concatenate([im, np.full(im.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
        pose = np.asarray(c2w.cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)
        if pose.ndim != 3 or pose.shape[0] != im.shape[0] or pose.shape[1:] not in ((3, 4), (4, 4)):
            raise ValueError(f"c2w must be [N,3,4] or [N,4,4] with N = {im.shape[0]}, got {pose.shape}")
        H, W = im.shape[1:3]
        nm = None
        if normals is not None:
            nm = np.asarray(normals.cpu() if isinstance(normals, torch.Tensor) else normals)
            if nm.shape != im.shape[:3] + (3,):
                raise ValueError(f"normals must be [N,H,W,3] = {im.shape[:3] + (3,)}, got {nm.shape}")
            if nm.dtype != np.uint8:
                nm = np.clip(np.rint((nm.astype(np.float64) * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
            nm = np.ascontiguousarray(nm)
        return cls(images=np.ascontiguousarray(im), c2w=np.ascontiguousarray(pose[:, :3, :4]), fx=float(focal),
                   fy=float(focal), cx=float(W / 2.0 if cx is None else cx), cy=float(H / 2.0 if cy is None else cy), normals=nm)


def load_blender_split(root: str, split: str, scale_factor: float = 1.0, normals: bool = False,
                       normals_suffix: str = "_normal") -> BlenderScene:
    """nerfstudio 0.3 BlenderDataParser: transforms_{split}.json; image = frame["file_path"] without a leading "./" plus
    ".png"; c2w = transform_matrix[:3] with the translation times scale_factor; fx = fy = 0.5 W / tan(0.5 camera_angle_x),
    cx = W / 2, cy = H / 2.

    normals=True also reads every frame's normal map, file_path + normals_suffix + ".png" (multinerf's naming of the Shiny Blender
    scenes: r_0.png beside r_0_normal.png), into scene.normals: its first three channels, an alpha channel of that file ignored.
    FileNotFoundError for a frame without one, ValueError for one of another size than the frame's image."""
    from PIL import Image

    meta_path = os.path.join(root, f"transforms_{split}.json")
    if not os.path.isfile(meta_path):
        raise FileNotFoundError(f"{meta_path}: no such file (a Blender-format scene has transforms_{{train,val,test}}.json)")
    with open(meta_path) as fh:
        meta = json.load(fh)
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError(f"{meta_path} lists no frames")
    images, poses, normal_maps = [], [], []
    for fr in frames:
        rel = fr["file_path"]
        if rel.startswith("./"):
            rel = rel[2:]
        path = os.path.join(root, rel + ".png")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: image of frame {len(images)} of {meta_path} not found")
        with Image.open(path) as img:
            im = np.asarray(img.convert("RGBA") if img.mode != "RGBA" else img, dtype=np.uint8)
        if images and im.shape != images[0].shape:
            raise ValueError(f"{path}: image size {im.shape[1]} x {im.shape[0]} differs from the split's first image "
                             f"({images[0].shape[1]} x {images[0].shape[0]}); all images of a split must be equal in size")
        if normals:
            npath = os.path.join(root, rel + normals_suffix + ".png")
            if not os.path.isfile(npath):
                raise FileNotFoundError(f"{npath}: normal map of frame {len(images)} of {meta_path} not found")
            with Image.open(npath) as img:
                nm = np.asarray(img.convert("RGB") if img.mode not in ("RGB", "RGBA") else img, dtype=np.uint8)[..., :3]
            if nm.shape[:2] != im.shape[:2]:
                raise ValueError(f"{npath}: normal map of {nm.shape[1]} x {nm.shape[0]} pixels beside an image of "
                                 f"{im.shape[1]} x {im.shape[0]}; a frame's normal map must have its image's size")
            normal_maps.append(nm)
        images.append(im)
        poses.append(np.asarray(fr["transform_matrix"], dtype=np.float32)[:3, :4])
    im = np.stack(images)
    c2w = np.stack(poses)
    c2w[:, :, 3] *= np.float32(scale_factor)
    H, W = im.shape[1:3]
    focal = 0.5 * W / math.tan(0.5 * float(meta["camera_angle_x"]))
    return BlenderScene(images=im, c2w=c2w, fx=focal, fy=focal, cx=W / 2.0, cy=H / 2.0,
                        normals=np.ascontiguousarray(np.stack(normal_maps)) if normals else None)


MAX_LEVELS = 5  # include/rsn.h RSN_PYRAMID_MAX_LEVELS: a 16 x 16 box keeps the integer sums of the blend below 2^24


def pyramid_layout(n_images: int, height: int, width: int, levels: int) -> Tuple[Tuple[Tuple[int, int], ...], Tuple[int, ...]]:
    """The pyramid of include/rsn.h ("image pyramids") for N images of height x width: -> (sizes, offsets) with sizes[l] = (H >> l,
    W >> l) for l = 0 .. levels-1 and offsets[l] = the first pixel of level l >= 1 in the one allocation (offsets[0] = 0 is unused:
    level 0 is the image set itself), offsets[levels] = its size in pixels.  ValueError for levels outside 1 .. 5 and for a size that
    2^(levels-1) does not divide; host arithmetic only."""
    levels = int(levels)
    if not 1 <= levels <= MAX_LEVELS:
        raise ValueError(f"levels = {levels}: need 1 to {MAX_LEVELS}")
    s = 1 << (levels - 1)
    if height % s or width % s:
        raise ValueError(f"images of {width} x {height} pixels: {levels} levels need a width and a height divisible by {s}")
    sizes = tuple((height >> l, width >> l) for l in range(levels))
    offsets = [0, 0]
    for l in range(1, levels):
        offsets.append(offsets[-1] + n_images * sizes[l][0] * sizes[l][1])
    return sizes, tuple(offsets[:levels + 1])


class RayDataManager:
    """Training batches and full-image ray bundles of a BlenderScene, on `device`.

    The images and poses are uploaded once.  next_train(step) draws num_rays_per_batch pixels uniformly with replacement
    over all images (Philox4x32-10 keyed by (seed, rank), counter (step, ray)), so a batch is a pure function of
    (seed, rank, step): a later rank of a data-parallel run gets its own stream by its rank alone.

    levels > 1: the images also exist at 1/2 .. 1/2^(levels-1) of their size (self.pyramid, built once on the device); a ray's level
    is drawn first, with probability 1 / levels, then its pixel within the level, from the same Philox words.  levels = 1 is the
    single-scale path: the same launches and bytes as without the argument."""

    def __init__(self, scene: BlenderScene, device, num_rays_per_batch: int = 1024, seed: int = 0, rank: int = 0, levels: int = 1):
        self.levels = int(levels)
        self.level_sizes, self.level_offsets = pyramid_layout(scene.num_images, scene.height, scene.width, self.levels)  # raises first
        self.scene = scene
        self.device = torch.device(device)
        self.num_rays_per_batch = int(num_rays_per_batch)
        self.seed = int(seed) & 0xFFFFFFFF
        self.rank = int(rank) & 0xFFFFFFFF
        self.images = torch.from_numpy(np.ascontiguousarray(scene.images)).to(self.device)
        self.c2w = torch.from_numpy(np.ascontiguousarray(scene.c2w, dtype=np.float32)).to(self.device)
        self.normals = None  # uint8 [N,H,W,3]: level 0 only, the pyramid builds no normal levels
        if scene.normals is not None:
            self.normals = torch.from_numpy(np.ascontiguousarray(scene.normals)).to(self.device)
        self._lib = _abi.load_library()
        self.pyramid = None  # fp32 [pixels of the levels >= 1, 3]
        if self.levels > 1:
            self.pyramid = torch.empty(self.level_offsets[-1], 3, device=self.device, dtype=torch.float32)
            _abi.check(self._lib.rsn_build_pyramid(scene.num_images, scene.height, scene.width, self.levels, _abi.ptr(self.images),
                                                   _abi.ptr(self.pyramid), self.pyramid.shape[0], self._stream()))

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def next_train(self, step: int) -> Tuple[RayBundle, Dict[str, torch.Tensor]]:
        """-> (RayBundle [R] with nears / fars None (the model's collider fills them), {"image": [R,3] white-blended
        rgb, "indices": int32 [R,3] = (image, y, x)}).  One kernel launch.  With levels > 1 the batch also holds "levels": int32
        [R], and (y, x) are pixel coordinates of the ray's own level."""
        s, R = self.scene, self.num_rays_per_batch
        flat = torch.empty(R * 10, device=self.device, dtype=torch.float32)  # one allocation, four views
        multi = self.levels > 1
        idx = torch.empty(R, 4 if multi else 3, device=self.device, dtype=torch.int32)  # multi: the levels ride behind the indices
        o, d, pa, rgb = (flat[0:3 * R].view(R, 3), flat[3 * R:6 * R].view(R, 3), flat[6 * R:7 * R].view(R, 1),
                         flat[7 * R:10 * R].view(R, 3))
        if not multi:
            _abi.check(self._lib.rsn_sample_camera_rays(
                s.num_images, s.height, s.width, _abi.ptr(self.images), _abi.ptr(self.c2w), s.fx, s.fy, s.cx, s.cy, R,
                self.seed, self.rank, int(step) & 0xFFFFFFFF, _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa), _abi.ptr(rgb),
                _abi.ptr(idx), self._stream()))
            rb = RayBundle(origins=o, directions=d, pixel_area=pa, camera_indices=idx[:, 0:1])
            return rb, {"image": rgb, "indices": idx}
        both = idx.view(-1)
        idx, lvl = both[:3 * R].view(R, 3), both[3 * R:]
        _abi.check(self._lib.rsn_sample_pyramid_rays(
            s.num_images, s.height, s.width, self.levels, _abi.ptr(self.images), _abi.ptr(self.pyramid), self.pyramid.shape[0],
            _abi.ptr(self.c2w), s.fx, s.fy, s.cx, s.cy, R, self.seed, self.rank, int(step) & 0xFFFFFFFF, _abi.ptr(o), _abi.ptr(d),
            _abi.ptr(pa), _abi.ptr(rgb), _abi.ptr(idx), _abi.ptr(lvl), self._stream()))
        rb = RayBundle(origins=o, directions=d, pixel_area=pa, camera_indices=idx[:, 0:1])
        return rb, {"image": rgb, "indices": idx, "levels": lvl}

    def _level(self, level: int) -> int:
        if not 0 <= level < self.levels:
            raise IndexError(f"level {level} of {self.levels}")
        return int(level)

    def level_intrinsics(self, level: int = 0) -> Tuple[float, float, float, float]:
        """(fx, fy, cx, cy) of the level's camera: the scene's over 2^level (exact: a power of two)."""
        s, k = self.scene, float(1 << self._level(level))
        return s.fx / k, s.fy / k, s.cx / k, s.cy / k

    def camera_ray_bundle(self, i: int, level: int = 0) -> RayBundle:
        """The [H,W] RayBundle of camera i (row-major), for Model.get_outputs_for_camera_ray_bundle; level l: the [H >> l, W >> l]
        bundle of the level's camera (the same pose, the intrinsics over 2^l)."""
        s = self.scene
        if not 0 <= i < s.num_images:
            raise IndexError(f"camera {i} of {s.num_images}")
        from .render import camera_rays

        (h, w), (fx, fy, cx, cy) = self.level_sizes[self._level(level)], self.level_intrinsics(level)
        rb = camera_rays(self.c2w[i], h, w, fx, fy, cx, cy, self.device)
        rb.camera_indices = torch.full((h, w, 1), i, device=self.device, dtype=torch.int32)
        return rb

    def image(self, i: int, level: int = 0) -> torch.Tensor:
        """Ground truth of camera i: [H,W,4] float32 RGBA in [0, 1] on the device, uint8 / 255 as nerfstudio's
        InputDataset forms it (get_image_metrics_and_images and get_loss_dict blend the alpha onto white).  level l >= 1: the
        pyramid's [H >> l, W >> l, 3] image, already blended onto white; a view, not a copy."""
        if self._level(level) == 0:
            return torch.from_numpy(self.scene.images[i].astype(np.float32) / np.float32(255.0)).to(self.device)
        if not 0 <= i < self.scene.num_images:
            raise IndexError(f"camera {i} of {self.scene.num_images}")
        h, w = self.level_sizes[level]
        first = self.level_offsets[level] + i * h * w
        return self.pyramid[first:first + h * w].view(h, w, 3)

    def normal_image(self, i: int) -> torch.Tensor:
        """Ground-truth normal map of camera i: uint8 [H,W,3] on the device, the bytes of the scene's normal image (n * 0.5 + 0.5);
        a view of the one upload, not a copy.  Level 0 only.  ValueError when the scene has no normal maps."""
        if self.normals is None:
            raise ValueError("the scene has no normal maps (load_blender_split(..., normals=True) or from_arrays(..., normals=...))")
        if not 0 <= i < self.scene.num_images:
            raise IndexError(f"camera {i} of {self.scene.num_images}")
        return self.normals[i]
