"""Posed image sets without nerfstudio: a Blender-format parser and a device-resident ray data manager.

`load_blender_split` follows nerfstudio 0.3's BlenderDataParser (the reference trains with it: reflect_sampling_nerf_config.py:36-41);
`RayDataManager.next_train` is the reference datamanager's next_train (reflect_sampling_nerf_datamanager.py:49-58: pixel sampler ->
pixel gather -> ray generator) as ONE launch of rsn_sample_camera_rays on the images uploaded once: no host work beyond the launch,
no device-to-host read.  The exact sampling and ray recipes are in include/rsn.h.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

from . import _abi
from .nerfstudio_compat import RayBundle


@dataclass
class BlenderScene:
    """One split of a posed image set: images uint8 [N,H,W,4] RGBA (alpha 255 for RGB sources), c2w float32 [N,3,4],
    one pinhole camera (fx, fy, cx, cy) shared by all images."""

    images: np.ndarray
    c2w: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float

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
    def from_arrays(cls, images, c2w, focal: float, cx=None, cy=None) -> "BlenderScene":
        """images [N,H,W,3|4] (uint8, or float in [0, 1] rounded to uint8), c2w [N,3,4] or [N,4,4]; fx = fy = focal,
        principal point at the image centre unless given."""
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
        return cls(images=np.ascontiguousarray(im), c2w=np.ascontiguousarray(pose[:, :3, :4]), fx=float(focal),
                   fy=float(focal), cx=float(W / 2.0 if cx is None else cx), cy=float(H / 2.0 if cy is None else cy))


def load_blender_split(root: str, split: str, scale_factor: float = 1.0) -> BlenderScene:
    """nerfstudio 0.3 BlenderDataParser: transforms_{split}.json; image = frame["file_path"] without a leading "./" plus
    ".png"; c2w = transform_matrix[:3] with the translation times scale_factor; fx = fy = 0.5 W / tan(0.5 camera_angle_x),
    cx = W / 2, cy = H / 2."""
    from PIL import Image

    meta_path = os.path.join(root, f"transforms_{split}.json")
    if not os.path.isfile(meta_path):
        raise FileNotFoundError(f"{meta_path}: no such file (a Blender-format scene has transforms_{{train,val,test}}.json)")
    with open(meta_path) as fh:
        meta = json.load(fh)
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError(f"{meta_path} lists no frames")
    images, poses = [], []
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
        images.append(im)
        poses.append(np.asarray(fr["transform_matrix"], dtype=np.float32)[:3, :4])
    im = np.stack(images)
    c2w = np.stack(poses)
    c2w[:, :, 3] *= np.float32(scale_factor)
    H, W = im.shape[1:3]
    focal = 0.5 * W / math.tan(0.5 * float(meta["camera_angle_x"]))
    return BlenderScene(images=im, c2w=c2w, fx=focal, fy=focal, cx=W / 2.0, cy=H / 2.0)


class RayDataManager:
    """Training batches and full-image ray bundles of a BlenderScene, on `device`.

    The images and poses are uploaded once.  next_train(step) draws num_rays_per_batch pixels uniformly with replacement
    over all images (Philox4x32-10 keyed by (seed, rank), counter (step, ray)), so a batch is a pure function of
    (seed, rank, step): a later rank of a data-parallel run gets its own stream by its rank alone."""

    def __init__(self, scene: BlenderScene, device, num_rays_per_batch: int = 1024, seed: int = 0, rank: int = 0):
        self.scene = scene
        self.device = torch.device(device)
        self.num_rays_per_batch = int(num_rays_per_batch)
        self.seed = int(seed) & 0xFFFFFFFF
        self.rank = int(rank) & 0xFFFFFFFF
        self.images = torch.from_numpy(np.ascontiguousarray(scene.images)).to(self.device)
        self.c2w = torch.from_numpy(np.ascontiguousarray(scene.c2w, dtype=np.float32)).to(self.device)
        self._lib = _abi.load_library()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def next_train(self, step: int) -> Tuple[RayBundle, Dict[str, torch.Tensor]]:
        """-> (RayBundle [R] with nears / fars None (the model's collider fills them), {"image": [R,3] white-blended
        rgb, "indices": int32 [R,3] = (image, y, x)}).  One kernel launch."""
        s, R = self.scene, self.num_rays_per_batch
        flat = torch.empty(R * 10, device=self.device, dtype=torch.float32)  # one allocation, four views
        idx = torch.empty(R, 3, device=self.device, dtype=torch.int32)
        o, d, pa, rgb = (flat[0:3 * R].view(R, 3), flat[3 * R:6 * R].view(R, 3), flat[6 * R:7 * R].view(R, 1),
                         flat[7 * R:10 * R].view(R, 3))
        _abi.check(self._lib.rsn_sample_camera_rays(
            s.num_images, s.height, s.width, _abi.ptr(self.images), _abi.ptr(self.c2w), s.fx, s.fy, s.cx, s.cy, R,
            self.seed, self.rank, int(step) & 0xFFFFFFFF, _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa), _abi.ptr(rgb),
            _abi.ptr(idx), self._stream()))
        rb = RayBundle(origins=o, directions=d, pixel_area=pa, camera_indices=idx[:, 0:1])
        return rb, {"image": rgb, "indices": idx}

    def camera_ray_bundle(self, i: int) -> RayBundle:
        """The [H,W] RayBundle of camera i (row-major), for Model.get_outputs_for_camera_ray_bundle."""
        s = self.scene
        if not 0 <= i < s.num_images:
            raise IndexError(f"camera {i} of {s.num_images}")
        from .render import camera_rays

        rb = camera_rays(self.c2w[i], s.height, s.width, s.fx, s.fy, s.cx, s.cy, self.device)
        rb.camera_indices = torch.full((s.height, s.width, 1), i, device=self.device, dtype=torch.int32)
        return rb

    def image(self, i: int) -> torch.Tensor:
        """Ground truth of camera i: [H,W,4] float32 RGBA in [0, 1] on the device, uint8 / 255 as nerfstudio's
        InputDataset forms it (get_image_metrics_and_images and get_loss_dict blend the alpha onto white)."""
        return torch.from_numpy(self.scene.images[i].astype(np.float32) / np.float32(255.0)).to(self.device)
