"""Posed image sets without nerfstudio: a Blender-format parser, a nerfstudio-format (capture) parser and a device-resident ray
data manager.

`load_blender_split` follows nerfstudio 0.3's BlenderDataParser (the reference trains with it: reflect_sampling_nerf_config.py:36-41);
`RayDataManager.next_train` is the reference datamanager's next_train (reflect_sampling_nerf_datamanager.py:49-58: pixel sampler ->
pixel gather -> ray generator) as ONE launch of rsn_sample_camera_rays on the images uploaded once: no host work beyond the launch,
no device-to-host read.  The exact sampling and ray recipes are in include/rsn.h.

`RayDataManager(..., levels=L)` with L > 1 is mip-NeRF's multi-scale protocol: rsn_build_pyramid forms every image at 1/2 .. 1/2^(L-1)
of its size once, next_train draws each ray's level with probability 1/L (rsn_sample_pyramid_rays, still one launch), and
camera_ray_bundle / image take a level.

`load_nerfstudio_split` reads a nerfstudio-format capture (one transforms.json, as ns-process-data writes it): per-frame intrinsics,
OpenCV radial and tangential distortion, JPEG or PNG images, nerfstudio's pose normalisation and train / eval split.  Its scene
carries a camera table (`cameras` [N,9]); with one, RayDataManager uploads the table once and draws its batches with
rsn_sample_capture_rays and its views with rsn_capture_rays_image (include/rsn.h, "captures"): distorted rays are made on the
device, one launch, no host read.  Without a table every call is the one it always was.

Opt-in arguments of `load_nerfstudio_split` read what a real ns-process-data directory also holds: masks (scene.masks; the data
manager then builds per-level live-pixel lists on the device, rsn_build_live_pixels, and draws only from them), OPENCV_FISHEYE
cameras (a 12-column table whose fisheye rows go through the equidistant model on the device) and the images_K directories of a
downscale factor.  A scene with neither masks nor a 12-column table makes the calls it made before.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi
from .nerfstudio_compat import RayBundle


@dataclass
class BlenderScene:
    """One split of a posed image set: images uint8 [N,H,W,4] RGBA (alpha 255 for RGB sources), c2w float32 [N,3,4],
    one pinhole camera (fx, fy, cx, cy) shared by all images.  normals: None, or the ground-truth normal maps uint8 [N,H,W,3], the
    bytes of the scene's normal images, encoding n * 0.5 + 0.5 (eval's geometry metrics read them; training never does).

    cameras: None (the shared pinhole above, and nothing else changes), or the camera table of a capture, float32 [N,9] with row i =
    (fx, fy, cx, cy, k1, k2, k3, p1, p2) of image i (include/rsn.h, "captures"); fx .. cy then repeat row 0's pinhole part, for the
    callers that want one representative camera (an orbit's field of view, the occupancy box).  dataparser_transform [3,4] float64 and
    dataparser_scale: what load_nerfstudio_split applied to the file's poses (None for other sources); file_paths: the frames' names.

    A table of 12 columns (LENS_CAMERA_COLUMNS) holds fisheye rows: k4, the model (0 perspective, 1 OpenCV fisheye) and a zero follow
    the nine.  masks: None, or uint8 [N,H,W] of 0 / 1: 1 = the pixel is live, it may be drawn into a training batch.
    depths: None, or float32 [N,H,W] depth maps in scene units (the poses' units), 0 = no measurement: z-depths along the camera
    axis unless the caller says otherwise (RayDataManager(depth_euclidean=True): distances along the ray)."""

    images: np.ndarray
    c2w: np.ndarray
    fx: float
    fy: float
    cx: float
    cy: float
    normals: Optional[np.ndarray] = None
    cameras: Optional[np.ndarray] = None
    dataparser_transform: Optional[np.ndarray] = None
    dataparser_scale: Optional[float] = None
    file_paths: Optional[List[str]] = None
    masks: Optional[np.ndarray] = None
    depths: Optional[np.ndarray] = None

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
    def from_arrays(cls, images, c2w, focal: float, cx=None, cy=None, normals=None, masks=None, depths=None) -> "BlenderScene":
        """images [N,H,W,3|4] (uint8, or float in [0, 1] rounded to uint8), c2w [N,3,4] or [N,4,4]; fx = fy = focal,
        principal point at the image centre unless given.  normals: None, or [N,H,W,3] normal maps -- uint8 taken as is, float unit
        vectors encoded as rint((n * 0.5 + 0.5) * 255) clipped to 0..255.  masks: None, or [N,H,W], non-zero = live (stored as 0 / 1).
        depths: None, or [N,H,W] depth maps in scene units, 0 = no measurement (stored as float32); ValueError for a negative or
        non-finite value."""
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
        mk = None
        if masks is not None:
            mk = np.asarray(masks.cpu() if isinstance(masks, torch.Tensor) else masks)
            if mk.shape != im.shape[:3]:
                raise ValueError(f"masks must be [N,H,W] = {im.shape[:3]}, got {mk.shape}")
            mk = np.ascontiguousarray((mk != 0).astype(np.uint8))
        dp = None
        if depths is not None:
            dp = np.asarray(depths.cpu() if isinstance(depths, torch.Tensor) else depths)
            if dp.shape != im.shape[:3]:
                raise ValueError(f"depths must be [N,H,W] = {im.shape[:3]}, got {dp.shape}")
            if not np.all(np.isfinite(dp)) or np.any(dp < 0):
                raise ValueError("depths must be finite and >= 0 (0 = no measurement)")
            dp = np.ascontiguousarray(dp.astype(np.float32))
        return cls(images=np.ascontiguousarray(im), c2w=np.ascontiguousarray(pose[:, :3, :4]), fx=float(focal),
                   fy=float(focal), cx=float(W / 2.0 if cx is None else cx), cy=float(H / 2.0 if cy is None else cy), normals=nm,
                   masks=mk, depths=dp)


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


# ------------------------------------------------------------------------------------------------ captures (nerfstudio format)
CAMERA_COLUMNS = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")  # a row of the camera table (include/rsn.h, "captures")
LENS_CAMERA_COLUMNS = CAMERA_COLUMNS + ("k4", "model", "pad")  # a row of a table with fisheye rows; model: 0 perspective, 1 fisheye
CAPTURE_CAMERA_MODELS = (None, "OPENCV", "PINHOLE")
FISHEYE_CAMERA_MODEL = "OPENCV_FISHEYE"
ORIENTATIONS = ("up", "none")
CENTERS = ("poses", "none")
EVAL_MODES = ("fraction", "all")
DATA_FORMATS = ("auto", "blender", "nerfstudio")
UNDISTORT_ITERATIONS = 10  # the kernel's count (rsn_camera.h)
UNDISTORT_MAX_RESIDUAL = 1e-9  # of the load-time check, in normalised image units


def distort_points(row, X, Y):
    """The OpenCV / COLMAP model of include/rsn.h ("captures") in float64: undistorted normalised (X, Y) -> distorted (Xd, Yd).
    row: the nine numbers of a camera-table row (only k1 .. p2 are read).  Image coordinates: x right, y down."""
    k1, k2, k3, p1, p2 = (float(v) for v in row[4:9])
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    r2 = X * X + Y * Y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return X * rad + 2.0 * p1 * X * Y + p2 * (r2 + 2.0 * X * X), Y * rad + p1 * (r2 + 2.0 * Y * Y) + 2.0 * p2 * X * Y


def undistort_points(row, Xd, Yd, iterations: int = UNDISTORT_ITERATIONS):
    """The kernel's solve in float64: Newton on the 2 x 2 system from (Xd, Yd), `iterations` steps, none skipped early; a step whose
    |det J| <= 1e-12 leaves the point where it is.  -> (X, Y)."""
    k1, k2, k3, p1, p2 = (float(v) for v in row[4:9])
    Xd, Yd = np.asarray(Xd, dtype=np.float64), np.asarray(Yd, dtype=np.float64)
    x, y = Xd.copy(), Yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        drad = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3))
        rx = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - Xd
        ry = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - Yd
        j11 = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
        j12 = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
        j22 = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
        det = j11 * j22 - j12 * j12
        ok = np.abs(det) > 1e-12
        safe = np.where(ok, det, 1.0)
        x = np.where(ok, x - (j22 * rx - j12 * ry) / safe, x)
        y = np.where(ok, y - (j11 * ry - j12 * rx) / safe, y)
    return x, y


def undistort_residual(row, height: int, width: int) -> float:
    """The largest |distort(solve(p)) - p| of the kernel's solve at the four corners and four edge midpoints of the outermost pixel
    centres -- where the radius, and with it the distortion, is largest.  inf when the solve left the finite numbers."""
    fx, fy, cx, cy = (float(v) for v in row[:4])
    xs = np.array([0.5, 0.5 * width, width - 0.5], dtype=np.float64)
    ys = np.array([0.5, 0.5 * height, height - 0.5], dtype=np.float64)
    px, py = (a.ravel() for a in np.meshgrid(xs, ys))
    keep = ~((px == xs[1]) & (py == ys[1]))  # not the centre
    Xd, Yd = (px[keep] - cx) / fx, (py[keep] - cy) / fy
    with np.errstate(all="ignore"):
        X, Y = undistort_points(row, Xd, Yd)
        bx, by = distort_points(row, X, Y)
        res = np.maximum(np.abs(bx - Xd), np.abs(by - Yd))
    return float(res.max()) if np.all(np.isfinite(res)) else math.inf


def fisheye_forward(row, theta):
    """OpenCV's equidistant fisheye model of include/rsn.h ("captures: masks and fisheye lenses") in float64: the angle theta from the
    optical axis -> theta_d, the distorted radius in normalised image units.  row: a 12-column row (k1, k2, k3 and k4 are read)."""
    k1, k2, k3, k4 = float(row[4]), float(row[5]), float(row[6]), float(row[9])
    t = np.asarray(theta, dtype=np.float64)
    t2 = t * t
    return t * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))


def fisheye_solve(row, theta_d, iterations: int = UNDISTORT_ITERATIONS):
    """The kernel's solve in float64, before its clip to [0, pi]: Newton from theta = theta_d, `iterations` steps, none skipped early;
    a step whose |derivative| <= 1e-12 leaves theta where it is."""
    k1, k2, k3, k4 = float(row[4]), float(row[5]), float(row[6]), float(row[9])
    td = np.asarray(theta_d, dtype=np.float64)
    th = td.copy()
    for _ in range(iterations):
        t2 = th * th
        f = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
        df = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))))
        ok = np.abs(df) > 1e-12
        th = np.where(ok, th - f / np.where(ok, df, 1.0), th)
    return th


def fisheye_residual(row, height: int, width: int) -> float:
    """undistort_residual for a fisheye row: the largest |forward(solve(theta_d)) - theta_d| at the four corners and four edge
    midpoints of the outermost pixel centres.  inf when a solve left the finite numbers or [0, pi], or when theta_d is not strictly
    increasing in theta up to the largest solved angle (256 steps): the image then folds inside its border, and a pixel has two rays."""
    fx, fy, cx, cy = (float(v) for v in row[:4])
    xs = np.array([0.5, 0.5 * width, width - 0.5], dtype=np.float64)
    ys = np.array([0.5, 0.5 * height, height - 0.5], dtype=np.float64)
    px, py = (a.ravel() for a in np.meshgrid(xs, ys))
    keep = ~((px == xs[1]) & (py == ys[1]))  # not the centre
    td = np.hypot((px[keep] - cx) / fx, (py[keep] - cy) / fy)
    with np.errstate(all="ignore"):
        th = fisheye_solve(row, td)
        res = np.abs(fisheye_forward(row, th) - td)
        if not (np.all(np.isfinite(res)) and np.all(np.isfinite(th)) and np.all(th >= 0.0) and np.all(th <= math.pi)):
            return math.inf
        if np.any(np.diff(fisheye_forward(row, np.linspace(0.0, float(th.max()), 257))) <= 0.0):
            return math.inf
    return float(res.max())


def rotation_onto_z(up) -> np.ndarray:
    """The rotation [3,3] that takes the unit vector `up` onto +z, by Rodrigues' formula about up x z: I + K + K^2 / (1 + c) with
    c = up . z.  up = -z (no axis is singled out): the turn of pi about x."""
    a = np.asarray(up, dtype=np.float64)
    a = a / np.linalg.norm(a)
    c = float(a[2])
    if c < -1.0 + 1e-8:
        return np.diag([1.0, -1.0, -1.0])
    v = np.cross(a, np.array([0.0, 0.0, 1.0]))
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + K @ K / (1.0 + c)


def auto_orient_and_center_poses(c2w, orientation: str = "up", center: str = "poses") -> Tuple[np.ndarray, np.ndarray]:
    """nerfstudio's auto_orient_and_center_poses for the two methods a capture uses, in float64: c2w [N,3,4] -> (transform @ c2w,
    transform [3,4]).  center "poses": the mean camera position goes to the origin; orientation "up": the normalised mean of the
    cameras' up axes, c2w[:, :3, 1], goes to +z.  transform = [R | -R t]."""
    if orientation not in ORIENTATIONS:
        raise ValueError(f"orientation = {orientation!r}: choose from {', '.join(ORIENTATIONS)}")
    if center not in CENTERS:
        raise ValueError(f"center = {center!r}: choose from {', '.join(CENTERS)}")
    P = np.asarray(c2w, dtype=np.float64)[:, :3, :4]
    t = P[:, :, 3].mean(axis=0) if center == "poses" else np.zeros(3)
    R = np.eye(3)
    if orientation == "up":
        up = P[:, :, 1].mean(axis=0)
        n = np.linalg.norm(up)
        if not n > 0.0:
            raise ValueError("orientation 'up': the cameras' up axes average to zero; use orientation 'none'")
        R = rotation_onto_z(up / n)
    transform = np.concatenate([R, -(R @ t)[:, None]], axis=1)
    out = np.einsum("ij,njk->nik", R, P)
    out[:, :, 3] += transform[:, 3]
    return out, transform


def capture_split_indices(n: int, split: str, train_split_fraction: float = 0.9, eval_mode: str = "fraction") -> np.ndarray:
    """nerfstudio's fraction split of n frames (sorted by name): num_train = ceil(n * fraction), i_train = linspace(0, n - 1,
    num_train) truncated to integers, the eval set its complement; "train" gets i_train, "val" and "test" the complement.
    eval_mode "all": every split gets every frame."""
    if eval_mode not in EVAL_MODES:
        raise ValueError(f"eval_mode = {eval_mode!r}: choose from {', '.join(EVAL_MODES)}")
    if split not in ("train", "val", "test"):
        raise ValueError(f"split = {split!r}: choose from train, val, test")
    every = np.arange(n)
    if eval_mode == "all":
        return every
    if not 0.0 < train_split_fraction <= 1.0:
        raise ValueError(f"train_split_fraction = {train_split_fraction}: need 0 < F <= 1")
    i_train = np.linspace(0, n - 1, int(math.ceil(n * train_split_fraction)), dtype=int)
    return i_train if split == "train" else np.setdiff1d(every, i_train)


def detect_data_format(root: str, data_format: str = "auto") -> str:
    """"nerfstudio" for a directory with transforms.json, "blender" for one with transforms_train.json or any other
    transforms_{split}.json (the former wins when both exist); data_format other than "auto" is returned as it is."""
    if data_format not in DATA_FORMATS:
        raise ValueError(f"data_format = {data_format!r}: choose from {', '.join(DATA_FORMATS)}")
    if data_format != "auto":
        return data_format
    if os.path.isfile(os.path.join(root, "transforms.json")):
        return "nerfstudio"
    if os.path.isdir(root) and any(n.startswith("transforms_") and n.endswith(".json") for n in os.listdir(root)):
        return "blender"
    raise FileNotFoundError(f"{root}: neither transforms.json (a nerfstudio-format capture) nor transforms_train.json (a Blender-format scene)")


def write_dataparser_transforms(path: str, transform, scale: float) -> None:
    """nerfstudio's dataparser_transforms.json: {"transform": [3][4], "scale": s}."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump({"transform": np.asarray(transform, dtype=np.float64).tolist(), "scale": float(scale)}, fh, indent=4)
        fh.write("\n")


def load_nerfstudio_split(root: str, split: str, scale_factor: float = 1.0, orientation: str = "up", center: str = "poses",
                          auto_scale: bool = True, train_split_fraction: float = 0.9, eval_mode: str = "fraction",
                          applied: Optional[Tuple[Sequence, float]] = None, pixels: bool = True, masks: bool = False,
                          fisheye: bool = False, downscale_factor: int = 1, depths: bool = False,
                          depth_unit_scale: float = 1e-3) -> BlenderScene:
    """One split of a nerfstudio-format capture, root/transforms.json, as nerfstudio's NerfstudioDataParser reads it; -> a scene
    with a camera table.  All arithmetic on the host in float64, rounded once to float32.

    Cameras: fl_x, fl_y, cx, cy, w, h, k1, k2, k3, p1, p2 globally or per frame (the frame's value wins), missing coefficients 0;
    camera_model absent, OPENCV or PINHOLE.  Frames are ordered by file_path (plain string sort); file_path is relative to the JSON
    and carries its extension; PNG and JPEG through Pillow, RGB images get alpha 255.
    Poses: auto_orient_and_center_poses over ALL frames (before the split), then the translations times scale_factor / max |t| --
    the largest absolute translation component, nerfstudio's rule -- when auto_scale is on, else times scale_factor.
    applied = (transform [3,4], scale): apply exactly these instead (a checkpoint's: the frame a model was trained in).
    Split: capture_split_indices.
    pixels=False: the images are not decoded, only their headers read (every check below still runs); scene.images is then a
    read-only zero-stride array of the right shape -- for a caller that wants the cameras alone (render).

    ValueError, naming the frame: another camera_model (OPENCV_FISHEYE, ...), a non-zero k4, a mask_path, images of differing
    sizes, a w / h that disagrees with the file, and a coefficient set whose solve does not converge over the image (residual above
    1e-9 at the corners and edge midpoints: the model is not invertible there; the kernels do not check).  FileNotFoundError for a
    missing image.  Masks, fisheye cameras and a non-zero k4 are refused in the same way unless the arguments below ask for them;
    images of differing sizes and equirectangular cameras always are.

    masks=True: a frame's mask_path (relative to the JSON, read through Pillow) says which of its pixels are live: those whose first
    channel is non-zero, nerfstudio's rule for its single-channel masks; a frame without one is all live.  scene.masks is uint8
    [N,H,W] of 0 / 1, or None when no kept frame has a mask (and with pixels=False).  ValueError naming the frame for a mask of
    another size than its image, FileNotFoundError naming the file for a missing one.
    fisheye=True: camera_model OPENCV_FISHEYE (k1 .. k4; p1 and p2 must be 0) is accepted, and k4 with it (a perspective row must
    keep k4 = 0).  When a kept frame is a fisheye one the table has 12 columns, LENS_CAMERA_COLUMNS; else the 9 it always had.  The
    invertibility check of a fisheye row is fisheye_residual, against the same 1e-9.
    downscale_factor=K > 1, nerfstudio's rule: images/frame.png is read from images_K/frame.png (the parent directory's name gets
    _K; a mask_path likewise), fl_x, fl_y, cx, cy are divided by K, and a declared w, h must be the file's size times K up to the
    truncation of w // K, h // K.  FileNotFoundError naming the directory when it is missing: nothing is resampled here.
    depths=True: a frame's depth_file_path (what ns-process-data polycam --use-depth and record3d write; relative to the JSON) is read
    as a 16-bit PNG (Pillow mode I;16 or I) or a .npy float array, and scene.depths is float32 [N,H,W] =
    raw * depth_unit_scale * s, s being the factor the translations were multiplied by above (scale_factor, over max |t| when
    auto_scale is on; applied's scale): the product is formed in float64 and rounded once; 0 = no measurement.
    depth_unit_scale = 1e-3 is nerfstudio's (millimetres).  scene.depths is None when no kept frame has the key (and with
    pixels=False, which still checks the files' presence).  ValueError naming the frame: a kept frame without the key when another
    has it, a file of another size than its image, of another kind than the two above, or with a negative or non-finite value;
    FileNotFoundError naming the frame for a missing file.  With downscale_factor = K the file comes from depths_K/ (the same
    folder rule); nothing is resampled.  depths=False (the default): the key is ignored."""
    from PIL import Image

    meta_path = os.path.join(root, "transforms.json")
    if not os.path.isfile(meta_path):
        raise FileNotFoundError(f"{meta_path}: no such file (a nerfstudio-format capture has one transforms.json)")
    with open(meta_path) as fh:
        meta = json.load(fh)
    frames = sorted(meta.get("frames") or [], key=lambda fr: fr["file_path"])
    if not frames:
        raise ValueError(f"{meta_path} lists no frames")

    def value(fr, key, default=None):
        v = fr.get(key, meta.get(key, default))
        if v is None:
            raise ValueError(f"{meta_path}: frame {fr['file_path']} has no {key}, and the file has no global one")
        return v

    K = int(downscale_factor)
    if K < 1 or K != downscale_factor:
        raise ValueError(f"downscale_factor = {downscale_factor}: need an integer >= 1")

    def on_disk(rel):  # nerfstudio: images/frame.png -> images_K/frame.png
        if K == 1:
            return os.path.join(root, rel)
        parent, base = os.path.split(rel)
        if not parent:
            raise ValueError(f"{meta_path}: {rel} lies in no directory whose name could get _{K} (downscale_factor = {K})")
        scaled = os.path.join(root, parent + f"_{K}")
        if not os.path.isdir(scaled):
            raise FileNotFoundError(f"{scaled}: no such directory; downscale_factor = {K} reads the {parent}_{K} that ns-process-data "
                                    "writes beside it, and nothing is resampled here")
        return os.path.join(scaled, base)

    rows, poses, fish, k4s = [], [], [], []
    for fr in frames:
        name = fr["file_path"]
        model = fr.get("camera_model", meta.get("camera_model"))
        fish.append(bool(fisheye) and model == FISHEYE_CAMERA_MODEL)
        if model not in CAPTURE_CAMERA_MODELS and not fish[-1]:
            raise ValueError(f"{meta_path}: frame {name}: camera_model {model!r} is not supported (OPENCV, PINHOLE or absent)")
        k4s.append(float(fr.get("k4", meta.get("k4", 0.0)) or 0.0))
        if k4s[-1] != 0.0 and not fisheye:
            raise ValueError(f"{meta_path}: frame {name}: k4 = {fr.get('k4', meta.get('k4'))} is not zero; the model here has k1, k2, k3, p1, p2")
        if k4s[-1] != 0.0 and not fish[-1]:
            raise ValueError(f"{meta_path}: frame {name}: k4 = {k4s[-1]} is not zero, and its camera_model {model!r} is a perspective "
                             "one; only OPENCV_FISHEYE has a k4")
        if "mask_path" in fr and not masks:
            raise ValueError(f"{meta_path}: frame {name} has a mask_path; masks are not supported")
        rows.append([float(value(fr, "fl_x")), float(value(fr, "fl_y")), float(value(fr, "cx")), float(value(fr, "cy"))]
                    + [float(value(fr, k, 0.0)) for k in CAMERA_COLUMNS[4:]])
        if rows[-1][0] == 0.0 or rows[-1][1] == 0.0:
            raise ValueError(f"{meta_path}: frame {name}: fl_x = {rows[-1][0]}, fl_y = {rows[-1][1]}: a focal length is zero")
        if fish[-1] and (rows[-1][7] != 0.0 or rows[-1][8] != 0.0):
            raise ValueError(f"{meta_path}: frame {name}: p1 = {rows[-1][7]}, p2 = {rows[-1][8]}: an OPENCV_FISHEYE camera has k1 .. k4 "
                             "and no tangential terms")
        poses.append(np.asarray(fr["transform_matrix"], dtype=np.float64)[:3, :4])
    rows64, poses = np.asarray(rows, dtype=np.float64), np.stack(poses)
    if K > 1:
        rows64[:, :4] /= float(K)
    lens64 = np.concatenate([rows64, np.asarray(k4s)[:, None], np.asarray(fish, dtype=np.float64)[:, None], np.zeros((len(rows), 1))], axis=1)
    if applied is None:
        poses, transform = auto_orient_and_center_poses(poses, orientation, center)
        scale = float(scale_factor)
        if auto_scale:
            scale /= float(np.abs(poses[:, :, 3]).max())
    else:
        transform, scale = np.asarray(applied[0], dtype=np.float64)[:3, :4], float(applied[1])
        poses = np.einsum("ij,njk->nik", transform[:, :3], poses)
        poses[:, :, 3] += transform[:, 3]
    poses[:, :, 3] *= scale

    keep = capture_split_indices(len(frames), split, train_split_fraction, eval_mode)
    if len(keep) == 0:
        raise ValueError(f"{meta_path}: the {split} split of {len(frames)} frames at train_split_fraction {train_split_fraction} is empty")
    images, size = [], None
    live = {}  # position among the kept frames -> uint8 [H,W]
    checked = {}
    depth_maps = []
    with_depth = [i for i in keep if "depth_file_path" in frames[i]] if depths else []
    if with_depth and len(with_depth) != len(keep):
        lacking = next(frames[i]["file_path"] for i in keep if "depth_file_path" not in frames[i])
        raise ValueError(f"{meta_path}: frame {lacking} has no depth_file_path, and frame {frames[with_depth[0]]['file_path']} of the same "
                         "split has one; depth supervision needs a depth file for every frame of the split or for none")
    for i in keep:
        fr, name = frames[i], frames[i]["file_path"]
        path = on_disk(name)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: image of frame {name} of {meta_path} not found")
        with Image.open(path) as img:
            if pixels:
                im = np.asarray(img.convert("RGBA") if img.mode != "RGBA" else img, dtype=np.uint8)
            else:
                im = np.broadcast_to(np.zeros(1, np.uint8), (img.size[1], img.size[0], 4))
        if size is None:
            size = im.shape[:2]
        if im.shape[:2] != size:
            raise ValueError(f"{meta_path}: frame {name} is {im.shape[1]} x {im.shape[0]} pixels, the split's first image "
                             f"{size[1]} x {size[0]}; images of differing sizes are not supported")
        w, h = fr.get("w", meta.get("w")), fr.get("h", meta.get("h"))
        if (w is not None and int(w) // K != im.shape[1]) or (h is not None and int(h) // K != im.shape[0]):
            raise ValueError(f"{meta_path}: frame {name}: w x h = {w} x {h}, but the file holds {im.shape[1]} x {im.shape[0]} pixels"
                             + ("" if K == 1 else f" (downscale_factor = {K}: {int(w) // K} x {int(h) // K} expected)"))
        if masks and "mask_path" in fr:
            mpath = on_disk(fr["mask_path"])
            if not os.path.isfile(mpath):
                raise FileNotFoundError(f"{mpath}: mask of frame {name} of {meta_path} not found")
            with Image.open(mpath) as img:
                if (img.size[1], img.size[0]) != tuple(im.shape[:2]):
                    raise ValueError(f"{meta_path}: frame {name}: its mask {fr['mask_path']} is {img.size[0]} x {img.size[1]} pixels, "
                                     f"the image {im.shape[1]} x {im.shape[0]}; a frame's mask must have its image's size")
                if pixels:
                    mk = np.asarray(img)
                    live[len(images)] = ((mk if mk.ndim == 2 else mk[..., 0]) != 0).astype(np.uint8)
        if with_depth:
            dpath = on_disk(fr["depth_file_path"])
            if not os.path.isfile(dpath):
                raise FileNotFoundError(f"{dpath}: depth file of frame {name} of {meta_path} not found")
            if dpath.lower().endswith(".npy"):
                raw = np.load(dpath, mmap_mode=None if pixels else "r", allow_pickle=False)
                if raw.ndim == 3 and raw.shape[-1] == 1:
                    raw = raw[..., 0]
                if not np.issubdtype(raw.dtype, np.floating) or raw.ndim != 2:
                    raise ValueError(f"{meta_path}: frame {name}: its depth file {fr['depth_file_path']} holds a {raw.dtype} array of "
                                     f"shape {raw.shape}; a .npy depth file is a float [H,W] array")
                dsize = raw.shape
            else:
                with Image.open(dpath) as img:
                    if img.mode not in ("I;16", "I"):
                        raise ValueError(f"{meta_path}: frame {name}: its depth file {fr['depth_file_path']} has Pillow mode {img.mode}; "
                                         "a depth image is a 16-bit PNG (mode I;16 or I)")
                    dsize = (img.size[1], img.size[0])
                    raw = np.asarray(img) if pixels else None
            if tuple(dsize) != tuple(im.shape[:2]):
                raise ValueError(f"{meta_path}: frame {name}: its depth file {fr['depth_file_path']} is {dsize[1]} x {dsize[0]} pixels, "
                                 f"the image {im.shape[1]} x {im.shape[0]}; a frame's depth map must have its image's size")
            if pixels:
                raw64 = np.asarray(raw, dtype=np.float64)
                if not np.all(np.isfinite(raw64)) or np.any(raw64 < 0):
                    raise ValueError(f"{meta_path}: frame {name}: its depth file {fr['depth_file_path']} holds a negative or non-finite "
                                     "value (0 = no measurement)")
                depth_maps.append((raw64 * float(depth_unit_scale) * scale).astype(np.float32))
        key = lens64[i].tobytes()
        if fish[i]:
            if key not in checked:
                checked[key] = fisheye_residual(lens64[i], im.shape[0], im.shape[1])
                if not checked[key] <= UNDISTORT_MAX_RESIDUAL:
                    raise ValueError(f"{meta_path}: frame {name}: the fisheye model (k1, k2, k3, k4) = {tuple(lens64[i, [4, 5, 6, 9]])} is "
                                     f"not invertible over the {im.shape[1]} x {im.shape[0]} image: {UNDISTORT_ITERATIONS} Newton steps leave "
                                     f"a residual of {checked[key]:.3g} at its border (at most {UNDISTORT_MAX_RESIDUAL:g}; inf: theta "
                                     "beyond pi, or an image that folds inside its border)")
        elif key not in checked and np.any(rows64[i, 4:] != 0.0):
            checked[key] = undistort_residual(rows64[i], im.shape[0], im.shape[1])
            if not checked[key] <= UNDISTORT_MAX_RESIDUAL:
                raise ValueError(f"{meta_path}: frame {name}: the distortion model (k1, k2, k3, p1, p2) = {tuple(rows64[i, 4:])} is not "
                                 f"invertible over the {im.shape[1]} x {im.shape[0]} image: {UNDISTORT_ITERATIONS} Newton steps leave a "
                                 f"residual of {checked[key]:.3g} at its border (at most {UNDISTORT_MAX_RESIDUAL:g})")
        images.append(im)
    cams = np.ascontiguousarray((lens64 if np.any(np.asarray(fish)[keep]) else rows64)[keep].astype(np.float32))
    mask_stack = None
    if live:
        mask_stack = np.ones((len(images),) + tuple(size), np.uint8)
        for at, mk in live.items():
            mask_stack[at] = mk
    stack = np.ascontiguousarray(np.stack(images)) if pixels else np.broadcast_to(np.zeros(1, np.uint8), (len(images),) + images[0].shape)
    return BlenderScene(images=stack, c2w=np.ascontiguousarray(poses[keep].astype(np.float32)),
                        fx=float(cams[0, 0]), fy=float(cams[0, 1]), cx=float(cams[0, 2]), cy=float(cams[0, 3]), cameras=cams,
                        dataparser_transform=transform, dataparser_scale=scale, file_paths=[frames[i]["file_path"] for i in keep],
                        masks=mask_stack, depths=np.ascontiguousarray(np.stack(depth_maps)) if depth_maps else None)


def shared_pinhole(scene: BlenderScene, what: str) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) for a caller that projects through ONE pinhole camera (the TSDF and point-cloud exports): the scene's own,
    or a camera table's when all its rows are equal and free of distortion.  ValueError naming `what` otherwise."""
    cams = scene.cameras
    if cams is not None and (np.any(cams[:, 4:] != 0.0) or np.any(cams != cams[0])):  # a fisheye row has model = 1 in column 10
        raise ValueError(f"{what} projects through one shared pinhole camera: it accepts a capture only when all its cameras are equal "
                         "and free of lens distortion, and this one's are not")
    return scene.fx, scene.fy, scene.cx, scene.cy


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
    single-scale path: the same launches and bytes as without the argument.

    A scene with a camera table (scene.cameras, a capture): the table is uploaded once, per level with the four intrinsics over 2^l,
    and next_train / camera_ray_bundle go through rsn_sample_capture_rays / rsn_capture_rays_image at every level count.  Without a
    table they make the calls they always made.

    A scene with masks: the per-level lists of live pixels (include/rsn.h, "captures: masks and fisheye lenses") are built on the
    device at construction -- counted, the counts read once, allocated exactly, filled -- and next_train draws only from them;
    ValueError for a level without a live pixel; live_lists=False uploads the masks and builds no lists (eval draws no batches, and
    next_train then draws from every pixel).  With masks or a 12-column table next_train goes through
    rsn_sample_capture_rays_live and the views through rsn_capture_rays_image2; still one launch and no host read per call.

    A scene with depth maps (scene.depths): they are uploaded once, depth_image(i) serves them, and next_train adds the batch's
    target distances along the normalised rays, "depth" float32 [R] with 0 = no target, to the batch and, as [R,1], to the bundle's
    metadata (where the training graph's opt-in depth term reads them): one more launch (rsn_gather_ray_depth), no host read, no
    atomics.  depth_euclidean: the maps hold distances along the ray, not z-depths; a table with a fisheye row needs it (ValueError
    at construction otherwise: such a camera has no z-plane beyond 90 degrees).  The pyramid builds no depth levels: with levels > 1
    only the level-0 rays of a batch get a target -- a design rule.  A scene without depths makes the calls it made before."""

    def __init__(self, scene: BlenderScene, device, num_rays_per_batch: int = 1024, seed: int = 0, rank: int = 0, levels: int = 1,
                 live_lists: bool = True, depth_euclidean: bool = False):
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
        self.cameras = None  # fp32 [levels, N, 9]: level l's table has fx, fy, cx, cy over 2^l (exact), the coefficients as they are
        if scene.cameras is not None:
            cams = np.ascontiguousarray(scene.cameras, dtype=np.float32)
            if cams.shape not in ((scene.num_images, len(CAMERA_COLUMNS)), (scene.num_images, len(LENS_CAMERA_COLUMNS))):
                raise ValueError(f"cameras must be [{scene.num_images},{len(CAMERA_COLUMNS)}] (or {len(LENS_CAMERA_COLUMNS)} columns, with "
                                 f"fisheye rows), got {cams.shape}")
            scale = np.ones((self.levels, 1, cams.shape[1]), np.float32)
            scale[:, 0, :4] = (0.5 ** np.arange(self.levels, dtype=np.float32))[:, None]
            self.cameras = torch.from_numpy(cams[None] * scale).to(self.device)
        self._lib = _abi.load_library()
        self.pyramid = None  # fp32 [pixels of the levels >= 1, 3]
        if self.levels > 1:
            self.pyramid = torch.empty(self.level_offsets[-1], 3, device=self.device, dtype=torch.float32)
            _abi.check(self._lib.rsn_build_pyramid(scene.num_images, scene.height, scene.width, self.levels, _abi.ptr(self.images),
                                                   _abi.ptr(self.pyramid), self.pyramid.shape[0], self._stream()))
        self.masks = None  # uint8 [N,H,W] of 0 / 1
        self.live = self.live_offsets = self.live_counts = None  # the lists (uint32 bits in int32 tensors), [levels+1] offsets; host counts
        if scene.masks is not None and live_lists:
            self._build_live_pixels(scene)
        elif scene.masks is not None:  # a caller that draws no batches (eval): the masks alone, for mask_image
            self.masks = torch.from_numpy(np.ascontiguousarray(scene.masks, dtype=np.uint8)).to(self.device)
        self.depths = None  # fp32 [N,H,W]: level 0 only, the pyramid builds no depth levels
        self.depth_euclidean = bool(depth_euclidean)
        self.has_fisheye = bool(scene.cameras is not None and scene.cameras.shape[1] == len(LENS_CAMERA_COLUMNS)
                                and np.any(scene.cameras[:, 10] != 0.0))
        if scene.depths is not None:
            dp = np.ascontiguousarray(scene.depths, dtype=np.float32)
            if dp.shape != (scene.num_images, scene.height, scene.width):
                raise ValueError(f"depths must be [{scene.num_images},{scene.height},{scene.width}], got {dp.shape}")
            if self.has_fisheye and not self.depth_euclidean:
                raise ValueError("the camera table holds a fisheye row and the depth maps are z-depths: a fisheye camera has no z-plane "
                                 "beyond 90 degrees; its depth maps must hold distances along the ray (depth_euclidean=True)")
            self.depths = torch.from_numpy(dp).to(self.device)

    def _build_live_pixels(self, scene: BlenderScene) -> None:
        mk = np.ascontiguousarray(scene.masks, dtype=np.uint8)
        if mk.shape != (scene.num_images, scene.height, scene.width):
            raise ValueError(f"masks must be [{scene.num_images},{scene.height},{scene.width}], got {mk.shape}")
        if self.cameras is None:  # the masked sampler reads a table: the shared pinhole as N equal rows without distortion (the same bits)
            row = np.float32([scene.fx, scene.fy, scene.cx, scene.cy, 0, 0, 0, 0, 0])
            scale = np.ones((self.levels, 1, len(CAMERA_COLUMNS)), np.float32)
            scale[:, 0, :4] = (0.5 ** np.arange(self.levels, dtype=np.float32))[:, None]
            self.cameras = torch.from_numpy(np.tile(row, (scene.num_images, 1))[None] * scale).to(self.device)
        self.masks = torch.from_numpy(mk).to(self.device)
        shape = (scene.num_images, scene.height, scene.width, self.levels)
        ws = torch.empty(max(1, self._lib.rsn_live_pixels_workspace_bytes(*shape) // 4), device=self.device, dtype=torch.int32)
        counts = torch.zeros(self.levels, device=self.device, dtype=torch.int32)
        _abi.check(self._lib.rsn_build_live_pixels(*shape, _abi.ptr(self.masks), None, 0, _abi.ptr(counts), _abi.ptr(ws),
                                                   ws.numel() * 4, self._stream()))
        host = counts.cpu().numpy().view(np.uint32).astype(np.int64)  # the one host read, at construction
        for l, c in enumerate(host):
            if c == 0:
                raise ValueError(f"the masks leave no live pixel at level {l} of {self.levels} (a level-l pixel is live when all "
                                 f"{1 << l} x {1 << l} pixels under it are): nothing could be drawn there")
        self.live_counts = tuple(int(c) for c in host)
        self.live = torch.empty(int(host.sum()), device=self.device, dtype=torch.int32)
        _abi.check(self._lib.rsn_build_live_pixels(*shape, _abi.ptr(self.masks), _abi.ptr(self.live), self.live.numel(), _abi.ptr(counts),
                                                   _abi.ptr(ws), ws.numel() * 4, self._stream()))
        offsets = np.concatenate([[0], np.cumsum(host)]).astype(np.uint32).view(np.int32)
        self.live_offsets = torch.from_numpy(offsets).to(self.device)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def ray_depth(self, indices: torch.Tensor, levels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> float32 [R]: the target distance along the normalised ray of the pixels indices int32 [R,3] = (image, y, x), 0 = no
        target (a stored 0, or a ray of a level above 0); rsn_gather_ray_depth, one launch.  ValueError without depth maps."""
        if self.depths is None:
            raise ValueError("the scene has no depth maps (load_nerfstudio_split(..., depths=True) or from_arrays(..., depths=...))")
        from . import ops

        s = self.scene
        return ops.gather_ray_depth(indices, levels, self.depths, None if self.cameras is None else self.cameras[0],
                                    (s.fx, s.fy, s.cx, s.cy), self.has_fisheye, self.depth_euclidean)

    def view_ray_depth(self, i: int) -> torch.Tensor:
        """-> float32 [H,W]: ray_depth of every pixel of camera i, what eval's depth metrics compare depth_fine with."""
        s = self.scene
        if not 0 <= i < s.num_images:
            raise IndexError(f"camera {i} of {s.num_images}")
        y, x = torch.meshgrid(torch.arange(s.height, device=self.device, dtype=torch.int32),
                              torch.arange(s.width, device=self.device, dtype=torch.int32), indexing="ij")
        idx = torch.stack([torch.full_like(y, i), y, x], dim=-1).reshape(-1, 3).contiguous()
        return self.ray_depth(idx).view(s.height, s.width)

    def depth_image(self, i: int) -> torch.Tensor:
        """The depth map of camera i as stored: float32 [H,W] on the device, scene units, 0 = no measurement; a view of the one
        upload.  Level 0 only.  ValueError when the scene has no depth maps."""
        if self.depths is None:
            raise ValueError("the scene has no depth maps (load_nerfstudio_split(..., depths=True) or from_arrays(..., depths=...))")
        if not 0 <= i < self.scene.num_images:
            raise IndexError(f"camera {i} of {self.scene.num_images}")
        return self.depths[i]

    def next_train(self, step: int) -> Tuple[RayBundle, Dict[str, torch.Tensor]]:
        """_draw(step); a scene with depth maps adds batch["depth"] float32 [R], the rays' target distances (ray_depth), and the same
        values as ray_bundle.metadata["depth"] [R,1]."""
        rb, batch = self._draw(step)
        if self.depths is not None:
            t = self.ray_depth(batch["indices"], batch.get("levels"))
            batch["depth"] = t
            rb.metadata = {"depth": t.view(-1, 1)}
        return rb, batch

    def _draw(self, step: int) -> Tuple[RayBundle, Dict[str, torch.Tensor]]:
        """-> (RayBundle [R] with nears / fars None (the model's collider fills them), {"image": [R,3] white-blended
        rgb, "indices": int32 [R,3] = (image, y, x)}).  One kernel launch.  With levels > 1 the batch also holds "levels": int32
        [R], and (y, x) are pixel coordinates of the ray's own level."""
        s, R = self.scene, self.num_rays_per_batch
        flat = torch.empty(R * 10, device=self.device, dtype=torch.float32)  # one allocation, four views
        multi = self.levels > 1
        idx = torch.empty(R, 4 if multi else 3, device=self.device, dtype=torch.int32)  # multi: the levels ride behind the indices
        o, d, pa, rgb = (flat[0:3 * R].view(R, 3), flat[3 * R:6 * R].view(R, 3), flat[6 * R:7 * R].view(R, 1),
                         flat[7 * R:10 * R].view(R, 3))
        if self.cameras is not None:
            lvl = None  # single-scale: the sampler takes no level pointer, and the batch is shaped as it always was
            if multi:
                both = idx.view(-1)
                idx, lvl = both[:3 * R].view(R, 3), both[3 * R:]
            if self.live is not None or self.cameras.shape[-1] != len(CAMERA_COLUMNS):
                _abi.check(self._lib.rsn_sample_capture_rays_live(
                    s.num_images, s.height, s.width, self.levels, _abi.ptr(self.images), _abi.ptr(self.pyramid),
                    self.pyramid.shape[0] if multi else 0, _abi.ptr(self.c2w), _abi.ptr(self.cameras), self.cameras.shape[-1],
                    _abi.ptr(self.live), _abi.ptr(self.live_offsets), R, self.seed, self.rank, int(step) & 0xFFFFFFFF, _abi.ptr(o),
                    _abi.ptr(d), _abi.ptr(pa), _abi.ptr(rgb), _abi.ptr(idx), _abi.ptr(lvl), self._stream()))
                rb = RayBundle(origins=o, directions=d, pixel_area=pa, camera_indices=idx[:, 0:1])
                return rb, ({"image": rgb, "indices": idx, "levels": lvl} if multi else {"image": rgb, "indices": idx})
            _abi.check(self._lib.rsn_sample_capture_rays(
                s.num_images, s.height, s.width, self.levels, _abi.ptr(self.images), _abi.ptr(self.pyramid),
                self.pyramid.shape[0] if multi else 0, _abi.ptr(self.c2w), _abi.ptr(self.cameras), R, self.seed, self.rank,
                int(step) & 0xFFFFFFFF, _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa), _abi.ptr(rgb), _abi.ptr(idx), _abi.ptr(lvl), self._stream()))
            rb = RayBundle(origins=o, directions=d, pixel_area=pa, camera_indices=idx[:, 0:1])
            return rb, ({"image": rgb, "indices": idx, "levels": lvl} if multi else {"image": rgb, "indices": idx})
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
        rb = camera_rays(self.c2w[i], h, w, fx, fy, cx, cy, self.device, camera=None if self.cameras is None else self.cameras[level, i])
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

    def mask_image(self, i: int) -> torch.Tensor:
        """The mask of camera i: uint8 [H,W] of 0 / 1 on the device (1 = live), a view of the one upload.  Level 0 only.  ValueError
        when the scene has no masks."""
        if self.masks is None:
            raise ValueError("the scene has no masks (load_nerfstudio_split(..., masks=True) or from_arrays(..., masks=...))")
        if not 0 <= i < self.scene.num_images:
            raise IndexError(f"camera {i} of {self.scene.num_images}")
        return self.masks[i]

    def normal_image(self, i: int) -> torch.Tensor:
        """Ground-truth normal map of camera i: uint8 [H,W,3] on the device, the bytes of the scene's normal image (n * 0.5 + 0.5);
        a view of the one upload, not a copy.  Level 0 only.  ValueError when the scene has no normal maps."""
        if self.normals is None:
            raise ValueError("the scene has no normal maps (load_blender_split(..., normals=True) or from_arrays(..., normals=...))")
        if not 0 <= i < self.scene.num_images:
            raise IndexError(f"camera {i} of {self.scene.num_images}")
        return self.normals[i]
