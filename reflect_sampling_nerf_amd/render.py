"""Pictures of a trained model from chosen viewpoints: camera paths, rays of an arbitrary pose, and the eval outputs drawn as
8-bit panels on the device (rsn_visualize, include/rsn.h).

    camera_rays        the [H,W] RayBundle of any pose, through the rays kernel of the data path (rsn_camera_rays_image)
    orbit_path / load_poses / interpolate_path
                       camera-to-world matrices [F,3,4] made on the host in fp64, returned as fp32
    draw_channels      eval outputs -> one uint8 panel, one launch per channel
    render_path        frames of a path: rays, the model's chunked eval render, the panel, an asynchronous copy to the host;
                       the consumer of frame i-1 (PNG encoding) runs beside the GPU work of frame i

Camera convention (the rays kernel's, nerfstudio's and Blender's): a camera looks along its -z axis, +y is up, +x is right; the
columns of c2w are [right, up, -forward, position].  World up is +z, as in Blender-format scenes.
"""
from __future__ import annotations

import json
import math
import os
import time
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _abi, ops
from ._abi import RSN_VIS_GRAY, RSN_VIS_LUT, RSN_VIS_RGB, RSN_VIS_UNIT
from ._host import replacing
from .checkpoint import open_checkpoint
from .nerfstudio_compat import RayBundle

# The turbo colour map (A. Mikhailov, Google, 2019; Apache-2.0), its published 256-entry table: what matplotlib ships as "turbo"
# and nerfstudio's depth colour map looks up.
TURBO = np.array([
    (0.18995, 0.07176, 0.23217), (0.19483, 0.08339, 0.26149), (0.19956, 0.09498, 0.29024), (0.20415, 0.10652, 0.31844),
    (0.20860, 0.11802, 0.34607), (0.21291, 0.12947, 0.37314), (0.21708, 0.14087, 0.39964), (0.22111, 0.15223, 0.42558),
    (0.22500, 0.16354, 0.45096), (0.22875, 0.17481, 0.47578), (0.23236, 0.18603, 0.50004), (0.23582, 0.19720, 0.52373),
    (0.23915, 0.20833, 0.54686), (0.24234, 0.21941, 0.56942), (0.24539, 0.23044, 0.59142), (0.24830, 0.24143, 0.61286),
    (0.25107, 0.25237, 0.63374), (0.25369, 0.26327, 0.65406), (0.25618, 0.27412, 0.67381), (0.25853, 0.28492, 0.69300),
    (0.26074, 0.29568, 0.71162), (0.26280, 0.30639, 0.72968), (0.26473, 0.31706, 0.74718), (0.26652, 0.32768, 0.76412),
    (0.26816, 0.33825, 0.78050), (0.26967, 0.34878, 0.79631), (0.27103, 0.35926, 0.81156), (0.27226, 0.36970, 0.82624),
    (0.27334, 0.38008, 0.84037), (0.27429, 0.39043, 0.85393), (0.27509, 0.40072, 0.86692), (0.27576, 0.41097, 0.87936),
    (0.27628, 0.42118, 0.89123), (0.27667, 0.43134, 0.90254), (0.27691, 0.44145, 0.91328), (0.27701, 0.45152, 0.92347),
    (0.27698, 0.46153, 0.93309), (0.27680, 0.47151, 0.94214), (0.27648, 0.48144, 0.95064), (0.27603, 0.49132, 0.95857),
    (0.27543, 0.50115, 0.96594), (0.27469, 0.51094, 0.97275), (0.27381, 0.52069, 0.97899), (0.27273, 0.53040, 0.98461),
    (0.27106, 0.54015, 0.98930), (0.26878, 0.54995, 0.99303), (0.26592, 0.55979, 0.99583), (0.26252, 0.56967, 0.99773),
    (0.25862, 0.57958, 0.99876), (0.25425, 0.58950, 0.99896), (0.24946, 0.59943, 0.99835), (0.24427, 0.60937, 0.99697),
    (0.23874, 0.61931, 0.99485), (0.23288, 0.62923, 0.99202), (0.22676, 0.63913, 0.98851), (0.22039, 0.64901, 0.98436),
    (0.21382, 0.65886, 0.97959), (0.20708, 0.66866, 0.97423), (0.20021, 0.67842, 0.96833), (0.19326, 0.68812, 0.96190),
    (0.18625, 0.69775, 0.95498), (0.17923, 0.70732, 0.94761), (0.17223, 0.71680, 0.93981), (0.16529, 0.72620, 0.93161),
    (0.15844, 0.73551, 0.92305), (0.15173, 0.74472, 0.91416), (0.14519, 0.75381, 0.90496), (0.13886, 0.76279, 0.89550),
    (0.13278, 0.77165, 0.88580), (0.12698, 0.78037, 0.87590), (0.12151, 0.78896, 0.86581), (0.11639, 0.79740, 0.85559),
    (0.11167, 0.80569, 0.84525), (0.10738, 0.81381, 0.83484), (0.10357, 0.82177, 0.82437), (0.10026, 0.82955, 0.81389),
    (0.09750, 0.83714, 0.80342), (0.09532, 0.84455, 0.79299), (0.09377, 0.85175, 0.78264), (0.09287, 0.85875, 0.77240),
    (0.09267, 0.86554, 0.76230), (0.09320, 0.87211, 0.75237), (0.09451, 0.87844, 0.74265), (0.09662, 0.88454, 0.73316),
    (0.09958, 0.89040, 0.72393), (0.10342, 0.89600, 0.71500), (0.10815, 0.90142, 0.70599), (0.11374, 0.90673, 0.69651),
    (0.12014, 0.91193, 0.68660), (0.12733, 0.91701, 0.67627), (0.13526, 0.92197, 0.66556), (0.14391, 0.92680, 0.65448),
    (0.15323, 0.93151, 0.64308), (0.16319, 0.93609, 0.63137), (0.17377, 0.94053, 0.61938), (0.18491, 0.94484, 0.60713),
    (0.19659, 0.94901, 0.59466), (0.20877, 0.95304, 0.58199), (0.22142, 0.95692, 0.56914), (0.23449, 0.96065, 0.55614),
    (0.24797, 0.96423, 0.54303), (0.26180, 0.96765, 0.52981), (0.27597, 0.97092, 0.51653), (0.29042, 0.97403, 0.50321),
    (0.30513, 0.97697, 0.48987), (0.32006, 0.97974, 0.47654), (0.33517, 0.98234, 0.46325), (0.35043, 0.98477, 0.45002),
    (0.36581, 0.98702, 0.43688), (0.38127, 0.98909, 0.42386), (0.39678, 0.99098, 0.41098), (0.41229, 0.99268, 0.39826),
    (0.42778, 0.99419, 0.38575), (0.44321, 0.99551, 0.37345), (0.45854, 0.99663, 0.36140), (0.47375, 0.99755, 0.34963),
    (0.48879, 0.99828, 0.33816), (0.50362, 0.99879, 0.32701), (0.51822, 0.99910, 0.31622), (0.53255, 0.99919, 0.30581),
    (0.54658, 0.99907, 0.29581), (0.56026, 0.99873, 0.28623), (0.57357, 0.99817, 0.27712), (0.58646, 0.99739, 0.26849),
    (0.59891, 0.99638, 0.26038), (0.61088, 0.99514, 0.25280), (0.62233, 0.99366, 0.24579), (0.63323, 0.99195, 0.23937),
    (0.64362, 0.98999, 0.23356), (0.65394, 0.98775, 0.22835), (0.66428, 0.98524, 0.22370), (0.67462, 0.98246, 0.21960),
    (0.68494, 0.97941, 0.21602), (0.69525, 0.97610, 0.21294), (0.70553, 0.97255, 0.21032), (0.71577, 0.96875, 0.20815),
    (0.72596, 0.96470, 0.20640), (0.73610, 0.96043, 0.20504), (0.74617, 0.95593, 0.20406), (0.75617, 0.95121, 0.20343),
    (0.76608, 0.94627, 0.20311), (0.77591, 0.94113, 0.20310), (0.78563, 0.93579, 0.20336), (0.79524, 0.93025, 0.20386),
    (0.80473, 0.92452, 0.20459), (0.81410, 0.91861, 0.20552), (0.82333, 0.91253, 0.20663), (0.83241, 0.90627, 0.20788),
    (0.84133, 0.89986, 0.20926), (0.85010, 0.89328, 0.21074), (0.85868, 0.88655, 0.21230), (0.86709, 0.87968, 0.21391),
    (0.87530, 0.87267, 0.21555), (0.88331, 0.86553, 0.21719), (0.89112, 0.85826, 0.21880), (0.89870, 0.85087, 0.22038),
    (0.90605, 0.84337, 0.22188), (0.91317, 0.83576, 0.22328), (0.92004, 0.82806, 0.22456), (0.92666, 0.82025, 0.22570),
    (0.93301, 0.81236, 0.22667), (0.93909, 0.80439, 0.22744), (0.94489, 0.79634, 0.22800), (0.95039, 0.78823, 0.22831),
    (0.95560, 0.78005, 0.22836), (0.96049, 0.77181, 0.22811), (0.96507, 0.76352, 0.22754), (0.96931, 0.75519, 0.22663),
    (0.97323, 0.74682, 0.22536), (0.97679, 0.73842, 0.22369), (0.98000, 0.73000, 0.22161), (0.98289, 0.72140, 0.21918),
    (0.98549, 0.71250, 0.21650), (0.98781, 0.70330, 0.21358), (0.98986, 0.69382, 0.21043), (0.99163, 0.68408, 0.20706),
    (0.99314, 0.67408, 0.20348), (0.99438, 0.66386, 0.19971), (0.99535, 0.65341, 0.19577), (0.99607, 0.64277, 0.19165),
    (0.99654, 0.63193, 0.18738), (0.99675, 0.62093, 0.18297), (0.99672, 0.60977, 0.17842), (0.99644, 0.59846, 0.17376),
    (0.99593, 0.58703, 0.16899), (0.99517, 0.57549, 0.16412), (0.99419, 0.56386, 0.15918), (0.99297, 0.55214, 0.15417),
    (0.99153, 0.54036, 0.14910), (0.98987, 0.52854, 0.14398), (0.98799, 0.51667, 0.13883), (0.98590, 0.50479, 0.13367),
    (0.98360, 0.49291, 0.12849), (0.98108, 0.48104, 0.12332), (0.97837, 0.46920, 0.11817), (0.97545, 0.45740, 0.11305),
    (0.97234, 0.44565, 0.10797), (0.96904, 0.43399, 0.10294), (0.96555, 0.42241, 0.09798), (0.96187, 0.41093, 0.09310),
    (0.95801, 0.39958, 0.08831), (0.95398, 0.38836, 0.08362), (0.94977, 0.37729, 0.07905), (0.94538, 0.36638, 0.07461),
    (0.94084, 0.35566, 0.07031), (0.93612, 0.34513, 0.06616), (0.93125, 0.33482, 0.06218), (0.92623, 0.32473, 0.05837),
    (0.92105, 0.31489, 0.05475), (0.91572, 0.30530, 0.05134), (0.91024, 0.29599, 0.04814), (0.90463, 0.28696, 0.04516),
    (0.89888, 0.27824, 0.04243), (0.89298, 0.26981, 0.03993), (0.88691, 0.26152, 0.03753), (0.88066, 0.25334, 0.03521),
    (0.87422, 0.24526, 0.03297), (0.86760, 0.23730, 0.03082), (0.86079, 0.22945, 0.02875), (0.85380, 0.22170, 0.02677),
    (0.84662, 0.21407, 0.02487), (0.83926, 0.20654, 0.02305), (0.83172, 0.19912, 0.02131), (0.82399, 0.19182, 0.01966),
    (0.81608, 0.18462, 0.01809), (0.80799, 0.17753, 0.01660), (0.79971, 0.17055, 0.01520), (0.79125, 0.16368, 0.01387),
    (0.78260, 0.15693, 0.01264), (0.77377, 0.15028, 0.01148), (0.76476, 0.14374, 0.01041), (0.75556, 0.13731, 0.00942),
    (0.74617, 0.13098, 0.00851), (0.73661, 0.12477, 0.00769), (0.72686, 0.11867, 0.00695), (0.71692, 0.11268, 0.00629),
    (0.70680, 0.10680, 0.00571), (0.69650, 0.10102, 0.00522), (0.68602, 0.09536, 0.00481), (0.67535, 0.08980, 0.00449),
    (0.66449, 0.08436, 0.00424), (0.65345, 0.07902, 0.00408), (0.64223, 0.07380, 0.00401), (0.63082, 0.06868, 0.00401),
    (0.61923, 0.06367, 0.00410), (0.60746, 0.05878, 0.00427), (0.59550, 0.05399, 0.00453), (0.58336, 0.04931, 0.00486),
    (0.57103, 0.04474, 0.00529), (0.55852, 0.04028, 0.00579), (0.54583, 0.03593, 0.00638), (0.53295, 0.03169, 0.00705),
    (0.51989, 0.02756, 0.00780), (0.50664, 0.02354, 0.00863), (0.49321, 0.01963, 0.00955), (0.47960, 0.01583, 0.01055),
], dtype=np.float32)


class Channel(NamedTuple):
    """One drawable quantity: `source` names the per-ray tensor (a key of the eval outputs, or "rendered_normals": ray_normals),
    `kind` the rsn_visualize kind, `lo` / `hi` its range (None: the caller's depth range), `alpha` the coverage laid over white."""

    source: str
    kind: int
    lo: Optional[float] = 0.0
    hi: Optional[float] = 1.0
    alpha: Optional[str] = None


CHANNELS: Dict[str, Channel] = {
    "rgb": Channel("mid_reflect_fine", RSN_VIS_RGB),
    "rgb_direct": Channel("mid_rgb_fine", RSN_VIS_RGB),
    "diffuse": Channel("diff", RSN_VIS_RGB),
    "tint": Channel("tint", RSN_VIS_RGB),
    "roughness": Channel("roughness", RSN_VIS_GRAY, 0.0, 1.0),
    "normals": Channel("rendered_normals", RSN_VIS_UNIT, alpha="accumulation_fine"),
    "depth": Channel("depth_fine", RSN_VIS_LUT, None, None, alpha="accumulation_fine"),
    "accumulation": Channel("accumulation_fine", RSN_VIS_GRAY, 0.0, 1.0),
    "mask": Channel("mask", RSN_VIS_GRAY, 0.0, 1.0),
}
DEFAULT_CHANNELS = ("rgb", "diffuse", "tint", "roughness", "normals", "depth", "accumulation")
MAX_ELEVATION_DEG = 89.9  # from here on the look direction is too close to world up for a stable `right`
DEFAULT_CHUNK = 4096  # rays per eval chunk: the kernels are at their best from 4096 rays; the reference evaluates 1024

_turbo_dev: Dict[torch.device, torch.Tensor] = {}


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _upload(host: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device through pinned memory, without waiting for the device."""
    return host.pin_memory().to(dev, non_blocking=True)


def _poses(c2w) -> np.ndarray:
    """One pose or a stack of them ([..,3,4] or [..,4,4]; tensor, array or nested lists) -> contiguous fp32 numpy [..,3,4]."""
    return np.ascontiguousarray(np.asarray(c2w.cpu() if isinstance(c2w, torch.Tensor) else c2w, dtype=np.float32)[..., :3, :4])


def turbo_lut(device) -> torch.Tensor:
    """TURBO on `device`, fp32 [256,3]; uploaded once per device."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    t = _turbo_dev.get(dev)
    if t is None:
        t = _turbo_dev[dev] = _upload(torch.from_numpy(TURBO), dev)
    return t


# ------------------------------------------------------------------------------------------------ rays
def camera_rays(c2w, height: int, width: int, fx: float, fy: float, cx: float, cy: float, device, camera=None) -> RayBundle:
    """The [H,W] RayBundle (origins, directions [H,W,3], pixel_area [H,W,1]; row-major) of the pinhole camera with pose c2w
    ([3,4] or [4,4]; a tensor on `device` is used where it lies, anything else is uploaded).  One launch, no host read.
    camera: None, or a camera row (fx, fy, cx, cy, k1, k2, k3, p1, p2) of a capture (include/rsn.h, "captures") -- nine numbers, or a
    fp32 tensor [9] on `device`, used where it lies; the view then goes through rsn_capture_rays_image and fx .. cy are not read.
    A row of 12 numbers (fx fy cx cy k1 k2 k3 p1 p2 k4 model 0: a capture with fisheye cameras) goes through rsn_capture_rays_image2."""
    dev = torch.device(device)
    there = isinstance(c2w, torch.Tensor) and c2w.device.type == dev.type
    pose = c2w[:3, :4].to(torch.float32).contiguous() if there else _upload(torch.from_numpy(_poses(c2w)), dev)
    H, W = int(height), int(width)
    flat = torch.empty(H * W * 7, device=dev, dtype=torch.float32)
    o, d, pa = flat[0:3 * H * W].view(H, W, 3), flat[3 * H * W:6 * H * W].view(H, W, 3), flat[6 * H * W:].view(H, W, 1)
    if camera is not None:
        if isinstance(camera, torch.Tensor) and camera.device.type == dev.type:
            row = camera.to(torch.float32).contiguous()
        else:
            row = _upload(torch.from_numpy(np.ascontiguousarray(np.asarray(camera.cpu() if isinstance(camera, torch.Tensor) else camera,
                                                                         dtype=np.float32))), dev)
        if tuple(row.shape) == (12,):
            _abi.check(_abi.load_library().rsn_capture_rays_image2(H, W, _abi.ptr(pose), _abi.ptr(row), 12, _abi.ptr(o), _abi.ptr(d),
                                                                   _abi.ptr(pa), _stream(dev)))
            return RayBundle(origins=o, directions=d, pixel_area=pa)
        if tuple(row.shape) != (9,):
            raise ValueError(f"camera must hold the 9 numbers fx fy cx cy k1 k2 k3 p1 p2 (or 12, with k4 model 0 behind them), got shape {tuple(row.shape)}")
        _abi.check(_abi.load_library().rsn_capture_rays_image(H, W, _abi.ptr(pose), _abi.ptr(row), _abi.ptr(o), _abi.ptr(d),
                                                              _abi.ptr(pa), _stream(dev)))
        return RayBundle(origins=o, directions=d, pixel_area=pa)
    _abi.check(_abi.load_library().rsn_camera_rays_image(H, W, _abi.ptr(pose), fx, fy, cx, cy, _abi.ptr(o), _abi.ptr(d),
                                                         _abi.ptr(pa), _stream(dev)))
    return RayBundle(origins=o, directions=d, pixel_area=pa)


def surface_maps(model, poses, H: int, W: int, fx: float, fy: float, cx: float, cy: float, views_per_launch: int = 8,
                 chunk: int = DEFAULT_CHUNK, accumulation: bool = False, events: Optional[list] = None):
    """The depth pass of mesh.fuse_depth and pointcloud.collect_points, a generator: the model's median depth (depth_fine of
    Model.get_surface_outputs) and, with `accumulation`, its accumulation_fine from the cameras poses [F,3,4] (or [F,4,4]) with one
    pinhole, views_per_launch views at a time, `chunk` rays per chunk.  Per launch it yields (start, poses_dev[start:start + n],
    depth[:n], acc[:n] or None): the maps are fp32 [n, H*W] views of one buffer that the next launch overwrites, to be used on the
    current stream before asking for the next.  F = 0 yields nothing.  No device-to-host read.
    events: a list that receives, per launch, a fresh list of two timing events, start and maps rendered; the consumer appends its own."""
    c2w = _poses(poses)
    F, H, W = len(c2w), int(H), int(W)
    views_per_launch = max(1, int(views_per_launch))
    dev = model.device
    poses_dev = _upload(torch.from_numpy(c2w), dev) if F else None
    depth = torch.empty(min(views_per_launch, max(F, 1)), H * W, device=dev, dtype=torch.float32)
    acc = torch.empty_like(depth) if accumulation else None
    for start in range(0, F, views_per_launch):
        n = min(views_per_launch, F - start)
        ev = ops.new_events(events)
        ops.record_event(ev)
        with torch.no_grad():
            for i in range(n):
                rays = camera_rays(poses_dev[start + i], H, W, fx, fy, cx, cy, dev)
                surf = model.get_surface_outputs_for_camera_ray_bundle(rays, chunk)
                depth[i] = surf["depth_fine"].reshape(H * W)
                if accumulation:
                    acc[i] = surf["accumulation_fine"].reshape(H * W)
        ops.record_event(ev)
        yield start, poses_dev[start:start + n], depth[:n], acc[:n] if accumulation else None


def camera_args(cameras: dict):
    """The cameras dict of the trainer's resolve_*_args -> (c2w, height, width, fx, fy, cx, cy), the order the functions take them in."""
    return tuple(cameras[k] for k in ("c2w", "height", "width", "fx", "fy", "cx", "cy"))


def pinhole(width: int, height: int, fov_x: float) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of the Blender-format camera: fov_x in radians (camera_angle_x), square pixels, centred."""
    f = 0.5 * width / math.tan(0.5 * fov_x)
    return f, f, width / 2.0, height / 2.0


# ------------------------------------------------------------------------------------------------ paths
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def orbit_path(frames: int, center, radius: float, elevation_deg: float, azimuth0_deg: float = 0.0) -> np.ndarray:
    """`frames` poses on a circle around `center` at `elevation_deg` above its xy-plane, all looking at `center`: position
    center + r (cos t cos p_i, cos t sin p_i, sin t) with p_i = azimuth0 + 2 pi i / frames (the last frame does not repeat the
    first); f = normalize(center - pos), right = normalize(f x z), up = right x f.  -> fp32 [F,3,4]."""
    if frames < 1:
        raise ValueError(f"frames must be >= 1, got {frames}")
    if not radius > 0.0:
        raise ValueError(f"radius must be > 0, got {radius}")
    if not abs(elevation_deg) < MAX_ELEVATION_DEG:
        raise ValueError(f"elevation {elevation_deg} deg: must be inside +-{MAX_ELEVATION_DEG} deg (the camera's `right` is "
                         "undefined when it looks along world up)")
    c = np.asarray(center, dtype=np.float64).reshape(3)
    th = math.radians(elevation_deg)
    ph = math.radians(azimuth0_deg) + 2.0 * math.pi * np.arange(frames, dtype=np.float64) / frames
    pos = c + radius * np.stack([math.cos(th) * np.cos(ph), math.cos(th) * np.sin(ph), np.full(frames, math.sin(th))], axis=1)
    f = _unit(c - pos)
    right = _unit(np.cross(f, np.array([0.0, 0.0, 1.0])))
    up = np.cross(right, f)
    return np.stack([right, up, -f, pos], axis=2).astype(np.float32)


def load_poses(json_path: str, scale_factor: float = 1.0) -> dict:
    """The cameras of a transforms-format file (a Blender-format transforms_*.json): {"c2w": fp32 [F,3,4] with the translation
    times scale_factor, "camera_angle_x", "width", "height", "file_paths"}; an entry the file does not have is None.  The images
    the frames name are not opened."""
    with open(json_path) as fh:
        meta = json.load(fh)
    frames = meta.get("frames") or []
    if not frames:
        raise ValueError(f"{json_path} lists no frames")
    c2w = np.stack([np.asarray(fr["transform_matrix"], dtype=np.float32)[:3, :4] for fr in frames])
    c2w[:, :, 3] *= np.float32(scale_factor)
    fov = meta.get("camera_angle_x")
    return {"c2w": np.ascontiguousarray(c2w), "camera_angle_x": None if fov is None else float(fov),
            "width": None if meta.get("w") is None else int(meta["w"]), "height": None if meta.get("h") is None else int(meta["h"]),
            "file_paths": [fr.get("file_path") for fr in frames]}


def _quaternion(R: np.ndarray) -> np.ndarray:
    """Unit quaternion (w, x, y, z) of a rotation matrix: the branch with the largest pivot (Shepperd)."""
    t = np.trace(R)
    if t > 0.0:
        s = math.sqrt(t + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(max(R[i, i] - R[j, j] - R[k, k] + 1.0, 0.0)) * 2.0
        q = np.empty(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def _rotation(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _slerp(q0: np.ndarray, q1: np.ndarray, t: float) -> np.ndarray:
    d = float(np.dot(q0, q1))
    if d < 0.0:  # q and -q are one rotation: take the shorter arc
        q1, d = -q1, -d
    if d > 1.0 - 1e-12:
        q = q0 + t * (q1 - q0)
    else:
        w = math.acos(d)
        q = (math.sin((1.0 - t) * w) * q0 + math.sin(t * w) * q1) / math.sin(w)
    return q / np.linalg.norm(q)


def interpolate_path(c2w, steps: int) -> np.ndarray:
    """`steps` poses between every two consecutive ones of c2w [F,3,4]: the rotation by quaternion slerp along the shorter arc, the
    translation linear.  The given poses are passed through untouched; steps = 0 returns them all.  -> fp32
    [(F-1)(steps+1)+1,3,4]."""
    src = _poses(c2w)
    if steps < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    if steps == 0 or len(src) < 2:
        return src.copy()
    quats = [_quaternion(p[:, :3].astype(np.float64)) for p in src]
    out = []
    for a in range(len(src) - 1):
        out.append(src[a])
        pa, pb = src[a, :, 3].astype(np.float64), src[a + 1, :, 3].astype(np.float64)
        for s in range(1, steps + 1):
            t = s / (steps + 1.0)
            pose = np.concatenate([_rotation(_slerp(quats[a], quats[a + 1], t)), ((1.0 - t) * pa + t * pb)[:, None]], axis=1)
            out.append(pose.astype(np.float32))
    out.append(src[-1])
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ drawing
def visualize(x: torch.Tensor, kind: int, out: torch.Tensor, x0: int = 0, alpha: Optional[torch.Tensor] = None, lo: float = 0.0,
              hi: float = 1.0, lut: Optional[torch.Tensor] = None) -> None:
    """rsn_visualize: x fp32 [H,W,3] (RGB, UNIT) or [H,W] / [H,W,1] (GRAY, LUT) into the tile [x0, x0 + W) of out, uint8
    [H,pitch,3]; alpha [H,W] / [H,W,1] or None.  All contiguous on one device; one launch on its current stream."""
    H, W = int(x.shape[0]), int(x.shape[1])
    want = H * W * (3 if kind in (RSN_VIS_RGB, RSN_VIS_UNIT) else 1)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != want:
        raise ValueError(f"x must be contiguous float32 with {want} elements for kind {kind}, got {x.dtype} {tuple(x.shape)}")
    if alpha is not None and (alpha.dtype != torch.float32 or not alpha.is_contiguous() or alpha.numel() != H * W):
        raise ValueError(f"alpha must be contiguous float32 with {H * W} elements, got {alpha.dtype} {tuple(alpha.shape)}")
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 3 or out.shape[0] != H or out.shape[2] != 3:
        raise ValueError(f"out must be contiguous uint8 [{H},pitch,3], got {out.dtype} {tuple(out.shape)}")
    if lut is not None and (lut.dtype != torch.float32 or not lut.is_contiguous() or tuple(lut.shape) != (256, 3)):
        raise ValueError(f"lut must be contiguous float32 [256,3], got {lut.dtype} {tuple(lut.shape)}")
    _abi.check(_abi.load_library().rsn_visualize(H, W, int(kind), _abi.ptr(x), _abi.ptr(alpha), float(lo), float(hi),
                                                 _abi.ptr(lut), _abi.ptr(out), int(out.shape[1]), int(x0), _stream(x.device)))


def ray_normals(outputs) -> torch.Tensor:
    """The composited predicted normal of every ray, normalize(sum_s w_s n_s), [...,3]: what the model's eval path renders for its
    reflect set-up but does not list among its outputs (the reference's key set stays as it is)."""
    n = (outputs["weights_fine"] * outputs["pred_normals_fine"]).sum(dim=-2)
    return torch.nn.functional.normalize(n, dim=-1)


def channel_tensor(outputs, source: str) -> torch.Tensor:
    """The contiguous fp32 tensor rsn_visualize reads for `source`."""
    if source == "rendered_normals":
        return ray_normals(outputs).contiguous()
    return outputs[source].to(torch.float32).contiguous()


def draw_channels(outputs, channels: Sequence[str], depth_range: Tuple[float, float], out: torch.Tensor, panel: bool = True) -> None:
    """One rsn_visualize per channel.  panel: out is uint8 [H, C*W, 3], the tiles left to right in the order of `channels`;
    else out is [C,H,W,3], one image per channel.  `outputs`: what get_outputs_for_camera_ray_bundle returned for the view."""
    alphas: Dict[str, torch.Tensor] = {}
    for c, name in enumerate(channels):
        ch = CHANNELS[name]
        x = channel_tensor(outputs, ch.source)
        W = int(x.shape[1])
        alpha = None
        if ch.alpha is not None:
            alpha = alphas.get(ch.alpha)
            if alpha is None:
                alpha = alphas[ch.alpha] = channel_tensor(outputs, ch.alpha)
        lo, hi = (depth_range if ch.lo is None else (ch.lo, ch.hi))
        lut = turbo_lut(x.device) if ch.kind == RSN_VIS_LUT else None
        if panel:
            visualize(x, ch.kind, out, c * W, alpha, lo, hi, lut)
        else:
            visualize(x, ch.kind, out[c], 0, alpha, lo, hi, lut)


def check_channels(channels: Sequence[str]) -> Tuple[str, ...]:
    bad = [c for c in channels if c not in CHANNELS]
    if bad or not channels:
        raise ValueError(f"unknown channel(s) {bad}: choose from {', '.join(CHANNELS)}")
    return tuple(channels)


def render_path(model, c2w, height: int, width: int, fx: float, fy: float, cx: float, cy: float,
                channels: Sequence[str] = DEFAULT_CHANNELS, depth_range: Optional[Tuple[float, float]] = None,
                on_frame: Optional[Callable[[int, np.ndarray], None]] = None, panel: bool = True,
                stage_events: Optional[list] = None, camera_table=None) -> List[np.ndarray]:
    """Render the poses c2w [F,3,4] with `model` (eval mode, on its device) and hand every frame to on_frame(i, array) in order.
    array is uint8 [H, C*W, 3] (panel: the channels' tiles left to right) or [C,H,W,3] (panel=False); it is a view of one of two
    pinned host buffers, valid until on_frame returns.  Without on_frame the frames are copied and returned as a list (with
    on_frame the list is empty).  depth_range: None = the model's collider planes.  camera_table: None, or one camera row per pose
    [F,9] (a capture's frames through their own cameras, lens distortion included); fx .. cy are then not read.

    Per frame i: rays, model.get_outputs_for_camera_ray_bundle, one rsn_visualize per channel, a non_blocking copy into host
    buffer i % 2 and an event.  Only after frame i is enqueued does the host wait for the event of frame i-1 and call its on_frame,
    so that frame's encoding runs beside the device work of frame i.  No threads, and no other host read.

    stage_events: a list that receives, per frame, five timing events recorded at: start, rays enqueued, render enqueued,
    panel drawn, copy enqueued (tools/render_path_report.py)."""
    channels = check_channels(channels)
    dev = model.device
    poses = _poses(c2w)
    F, H, W, C = len(poses), int(height), int(width), len(channels)
    if depth_range is None:
        depth_range = (float(model.config.collider_params["near_plane"]), float(model.config.collider_params["far_plane"]))
    lo, hi = float(depth_range[0]), float(depth_range[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
        raise ValueError(f"depth_range {depth_range}: need finite near < far")
    shape = (H, C * W, 3) if panel else (C, H, W, 3)
    poses_dev = _upload(torch.from_numpy(poses), dev)
    table_dev = None
    if camera_table is not None:
        table = np.ascontiguousarray(camera_table, dtype=np.float32)
        if table.shape not in ((F, 9), (F, 12)):
            raise ValueError(f"camera_table must be [{F},9] (or [{F},12] with fisheye rows), one row per pose, got {table.shape}")
        table_dev = _upload(torch.from_numpy(table), dev)
    panel_dev = torch.empty(shape, device=dev, dtype=torch.uint8)
    host = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(min(2, F))]
    done = [torch.cuda.Event() for _ in host]
    frames: List[np.ndarray] = []

    def deliver(i: int) -> None:
        done[i % 2].synchronize()
        arr = host[i % 2].numpy()
        if on_frame is None:
            frames.append(arr.copy())
        else:
            on_frame(i, arr)

    with torch.no_grad():
        for i in range(F):
            ev = ops.new_events(stage_events)
            ops.record_event(ev)
            rays = camera_rays(poses_dev[i], H, W, fx, fy, cx, cy, dev, camera=None if table_dev is None else table_dev[i])
            ops.record_event(ev)
            outputs = model.get_outputs_for_camera_ray_bundle(rays)
            ops.record_event(ev)
            draw_channels(outputs, channels, (lo, hi), panel_dev, panel)
            ops.record_event(ev)
            host[i % 2].copy_(panel_dev, non_blocking=True)
            done[i % 2].record()
            ops.record_event(ev)
            del outputs, rays
            if i > 0:
                deliver(i - 1)
        if F > 0:
            deliver(F - 1)
    return frames


# ------------------------------------------------------------------------------------------------ checkpoint -> frames
def render_checkpoint(ckpt: str, out_dir: str, c2w, height: int, width: int, fx: float, fy: float, cx: float, cy: float,
                      channels: Sequence[str] = DEFAULT_CHANNELS, depth_range: Optional[Tuple[float, float]] = None,
                      mma: str = "f32", chunk: int = DEFAULT_CHUNK, tiles: bool = False, device="cuda:0", model_config=None,
                      occupancy: Optional[dict] = None, camera_table=None) -> dict:
    """Render the poses c2w [F,3,4] from a checkpoint (a step-*.ckpt, or the newest of a run directory) into out_dir: the tiled
    panel of every frame as out_dir/panel/0000.png ..., or with `tiles` one image per channel as out_dir/<channel>/0000.png ...,
    and out_dir/frames.json (checkpoint, step, size, intrinsics, channels in tile order, depth range, mma, chunk, and per frame
    its file name(s) and c2w).  Existing files of these names are replaced; nothing else in out_dir is touched.
    occupancy: None, or {"resolution", "sigma", "dilate", "bounds" (None: occupancy.segment_bounds of the path)}: the frames are
    rendered with empty-space skipping and frames.json gains an "occupancy" entry (settings, box, occupied share of cells, culled
    share of rays; the latter read from the device once, after the last frame).  With "samples": True in it the field is also
    evaluated only on the samples in occupied cells, and the entry holds "samples": per level the sample slots seen and the live ones.
    camera_table: None, or [F,9], one camera row per pose (render_path); frames.json then holds every frame's row as "camera", and
    the occupancy box is laid out from the pinhole fx .. cy given here.
    -> the dict written to frames.json plus {"seconds": wall time of the frames, "out": out_dir}."""
    from PIL import Image

    channels = check_channels(channels)
    if chunk < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    ckpt, model, step = open_checkpoint(ckpt, model_config, torch.device(device), mma)
    model.config.eval_num_rays_per_chunk = int(chunk)
    if depth_range is None:
        depth_range = (model.config.collider_params["near_plane"], model.config.collider_params["far_plane"])
    poses = _poses(c2w)
    if occupancy is not None:
        from .occupancy import attach_occupancy

        attach_occupancy(model, occupancy, poses, height, width, fx, fy, cx, cy)
    folders = list(channels) if tiles else ["panel"]
    for f in folders:
        os.makedirs(os.path.join(out_dir, f), exist_ok=True)
    files: List[dict] = []

    def write(i: int, arr: np.ndarray) -> None:
        name = f"{i:04d}.png"
        if tiles:
            for c, ch in enumerate(channels):
                Image.fromarray(arr[c]).save(os.path.join(out_dir, ch, name))
            files.append({ch: f"{ch}/{name}" for ch in channels})
        else:
            Image.fromarray(arr).save(os.path.join(out_dir, "panel", name))
            files.append({"panel": f"panel/{name}"})

    t0 = time.time()
    render_path(model, poses, height, width, fx, fy, cx, cy, channels, depth_range, write, panel=not tiles, camera_table=camera_table)
    seconds = time.time() - t0
    meta = {"checkpoint": ckpt, "step": step, "width": int(width), "height": int(height), "fx": float(fx), "fy": float(fy),
            "cx": float(cx), "cy": float(cy), "channels": list(channels), "tiles": bool(tiles),
            "depth_range": [float(depth_range[0]), float(depth_range[1])], "mma": mma, "chunk": int(chunk),
            "frames": [{"files": f, "c2w": poses[i].astype(np.float64).tolist()} for i, f in enumerate(files)]}
    if camera_table is not None:
        for fr, row in zip(meta["frames"], np.asarray(camera_table, dtype=np.float64)):
            fr["camera"] = row.tolist()
    if occupancy is not None:
        meta["occupancy"] = model.occupancy.describe()
    with replacing(os.path.join(out_dir, "frames.json")) as tmp, open(tmp, "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    return {**meta, "seconds": seconds, "out": out_dir}
