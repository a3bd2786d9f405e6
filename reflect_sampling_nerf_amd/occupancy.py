"""Empty-space skipping for eval renders: an occupancy grid of the trained field, and the rays whose segment crosses no occupied
cell (rsn_occupancy_build / rsn_occupancy_cull / rsn_scatter_rows of include/rsn.h).

    build_occupancy    density_grid of the field -> one bit per grid cell (occupied: a corner with sigma >= threshold, grown by
                       `dilate` cells)
    segment_bounds     a box that holds the [near, far] segments of every ray of a set of pinhole cameras
    cull / scatter_rows   the two launches around the model's eval pipeline
    mark_and_compact / scatter_level   the same per SAMPLE of a level (rsn_occupancy_compact_samples / rsn_scatter_level): the
                       field is evaluated only on the samples whose interval crosses an occupied cell

`model.occupancy = grid` turns it on for the eval-mode get_outputs and get_outputs_for_camera_ray_bundle of
ReflectSamplingNeRFModel (None, the default, leaves that path exactly as it is; training never uses the grid).  Nothing here reads
the device: the number of hit rays stays in device memory and the later launches take it from there.

The defaults (sigma 0.01, one cell of dilation) are starting points from ONE experiment on a field trained for 2000 steps; they
have not been measured against a scene.  What the grid's box does not cover counts as occupied by default, so a box that is too
small costs speed, never correctness.

`model.occupancy_samples = True` (off by default; needs the grid) adds the per-sample decision: every level of the eval pipeline
goes through Field.evaluate_frustums_skipping.  A skipped sample gets sigma 0, hence weight 0.  A sample is kept, whatever cells it
crosses, when its cone is wider than sample_max_radius(grid) = max(dilate, 1) * min(spacing): dilation grew the occupied region by
that many cells, so a Gaussian narrower than the margin that sits in an unmarked cell has its bulk outside every above-threshold
cell.  That margin is a DESIGN RULE, reasoned and not measured: like sigma and the dilation it has not been tuned against a scene.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _abi, mesh, ops
from ._abi import check, ptr

DEFAULT_RESOLUTION = 128
DEFAULT_SIGMA = 0.01   # a starting point, not measured against any scene
DEFAULT_DILATE = 1     # likewise
BOUNDS_LATTICE = 33    # image-plane points per axis that segment_bounds shoots rays through
LEVELS = ("coarse", "fine", "reflect_coarse", "reflect_fine")  # level_id of the per-sample counters


def sample_max_radius(grid) -> float:
    """The widest cone radius a sample may have and still be skipped: the grid's dilation margin, max(dilate, 1) cells of the
    smallest spacing.  A design rule, not a measured value (see the module's docstring)."""
    return float(max(grid.dilate, 1)) * float(np.min(grid.spacing))


class OccupancyGrid:
    """One bit per cell of a regular grid (layout: include/rsn.h) on a device, with the frame and the settings it was built from.
    `rays_seen` (host) and `hits_dev` (device int64) count the rays culling has looked at and flagged; culled_share() reads the
    latter -- the only device-to-host read, meant for after the last frame."""

    def __init__(self, bits: Tensor, dims: Sequence[int], origin, spacing, threshold: float = DEFAULT_SIGMA,
                 dilate: int = DEFAULT_DILATE, outside_occupied: bool = True):
        self.dims = tuple(int(n) for n in dims)
        need = int(_abi.load_library().rsn_occupancy_bytes(*self.dims))
        if need == 0:
            check(-1)
        if bits.dtype != torch.int32 or not bits.is_contiguous() or bits.numel() * 4 != need or bits.device.type != "cuda":
            raise ValueError(f"bits must be a contiguous int32 tensor of {need // 4} words on a cuda (ROCm) device, got {bits.dtype} "
                             f"{tuple(bits.shape)} on {bits.device}")
        self.bits = bits
        self.origin = np.asarray(origin, dtype=np.float32).reshape(3).copy()
        self.spacing = np.asarray(spacing, dtype=np.float32).reshape(3).copy()
        self.threshold, self.dilate, self.outside_occupied = float(threshold), int(dilate), bool(outside_occupied)
        self._origin3, self._spacing3 = _abi.float3(self.origin), _abi.float3(self.spacing)
        self.rays_seen = 0
        self.hits_dev = torch.zeros(1, device=bits.device, dtype=torch.int64)
        # per-sample skipping, one entry per level (LEVELS): the sample slots its launches covered -- rows behind a device-side
        # count included, which are never live -- and, per stream that ran them, the live samples among them
        self.samples_seen = [0, 0, 0, 0]
        self._samples_live: Dict[int, Tensor] = {}
        self.sample_stage_events = None  # a list: every evaluate_frustums_skipping appends (level, [4 events]) (tools/occupancy_report.py)

    @property
    def n_cells(self) -> int:
        nx, ny, nz = self.dims
        return (nx - 1) * (ny - 1) * (nz - 1)

    @property
    def bounds(self) -> Tuple[float, ...]:
        hi = self.origin.astype(np.float64) + self.spacing.astype(np.float64) * (np.asarray(self.dims) - 1)
        return tuple(float(x) for x in (*self.origin, *hi))

    def occupied_share(self) -> float:
        """Occupied cells / all cells (copies the bits to the host)."""
        words = self.bits.cpu().numpy().view(np.uint32)
        return float(np.unpackbits(words.view(np.uint8)).sum()) / self.n_cells

    def culled_share(self) -> float:
        """Culled rays / rays seen since the grid was made (one device-to-host read)."""
        return 1.0 - int(self.hits_dev.item()) / self.rays_seen if self.rays_seen else 0.0

    @property
    def samples_live_dev(self) -> Tensor:
        """Live samples per level since the grid was made, device int64 [4].  The chunks of an image run on side streams, and every
        stream adds to a counter of its own (no atomics); this sums them on the current stream, which the model's calls have
        joined with the side streams by the time they return."""
        total = torch.zeros(len(LEVELS), device=self.bits.device, dtype=torch.int64)
        for acc in self._samples_live.values():
            total += acc
        return total

    def count_samples(self, level_id: int, seen: int, n_live: Tensor) -> None:
        """Book one rsn_occupancy_compact_samples: `seen` sample slots (host) and its device-side live count."""
        self.samples_seen[level_id] += int(seen)
        key = torch.cuda.current_stream(self.bits.device).cuda_stream
        acc = self._samples_live.get(key)
        if acc is None:
            acc = self._samples_live[key] = torch.zeros(len(LEVELS), device=self.bits.device, dtype=torch.int64)
        acc[level_id:level_id + 1] += n_live

    def describe(self) -> dict:
        """What `render` / `eval` record under "occupancy"; with per-sample skipping also "samples": per level the sample slots
        seen and the live ones (this and culled_share are the only host reads)."""
        d = {"resolution": list(self.dims), "sigma": self.threshold, "dilate": self.dilate, "outside_occupied": self.outside_occupied,
             "bounds": list(self.bounds), "occupied_share": self.occupied_share(), "culled_share": self.culled_share(),
             "rays": int(self.rays_seen)}
        if any(self.samples_seen):
            live = [int(x) for x in self.samples_live_dev.tolist()]
            d["samples"] = {"max_radius": sample_max_radius(self),
                            "levels": {name: {"seen": int(self.samples_seen[i]), "live": live[i]} for i, name in enumerate(LEVELS)}}
        return d


def occupancy_from_volume(vol: Tensor, origin, spacing, threshold: float = DEFAULT_SIGMA, dilate: int = DEFAULT_DILATE,
                          outside_occupied: bool = True) -> OccupancyGrid:
    """rsn_occupancy_build on a device volume fp32 [nz, ny, nx] (x fastest; vertex (i, j, k) at origin + spacing * (i, j, k))."""
    if vol.dim() != 3 or vol.dtype != torch.float32 or vol.device.type != "cuda":
        raise _abi.RsnError("occupancy_from_volume: vol must be an fp32 [nz, ny, nx] tensor on a cuda (ROCm) device")
    lib = _abi.load_library()
    vol = vol.contiguous()
    nz, ny, nx = (int(n) for n in vol.shape)
    nbytes = int(lib.rsn_occupancy_bytes(nx, ny, nz))
    if nbytes == 0:
        check(-1)
    bits = torch.empty(nbytes // 4, device=vol.device, dtype=torch.int32)
    with torch.cuda.device(vol.device):
        check(lib.rsn_occupancy_build(nx, ny, nz, ptr(vol), float(threshold), int(dilate), ptr(bits), nbytes, ops._stream()))
    return OccupancyGrid(bits, (nx, ny, nz), origin, spacing, threshold, dilate, outside_occupied)


def build_occupancy(field, bounds: Sequence[float], resolution: Union[int, Sequence[int]] = DEFAULT_RESOLUTION,
                    sigma: float = DEFAULT_SIGMA, dilate: int = DEFAULT_DILATE, outside_occupied: bool = True,
                    chunk: int = mesh.DEFAULT_CHUNK, mma: Optional[str] = None) -> OccupancyGrid:
    """The occupancy grid of a trained field over the box `bounds` = (x0, y0, z0, x1, y1, z1): mesh.density_grid (the field's sigma
    at every grid vertex, queried with one voxel's footprint) and rsn_occupancy_build.  The box should hold the [near, far]
    segments of the rays that will be culled (segment_bounds); with outside_occupied (the default) whatever it misses is rendered
    as before."""
    if dilate not in (0, 1, 2):
        raise ValueError(f"dilate must be 0, 1 or 2, got {dilate}")
    _, origin, spacing = mesh.grid_frame(bounds, resolution)
    vol = mesh.density_grid(field, bounds, resolution, chunk, mma)
    return occupancy_from_volume(vol, origin, spacing, sigma, dilate, outside_occupied)


def segment_bounds(c2w, height: int, width: int, fx: float, fy: float, cx: float, cy: float, near: float, far: float,
                   resolution: int = DEFAULT_RESOLUTION) -> Tuple[float, ...]:
    """A box (x0, y0, z0, x1, y1, z1) that holds the segment [near, far] of every pixel's ray of the pinhole cameras c2w [F,3,4]
    (the convention of render.camera_rays: unit directions).

    The far cap of a pinhole camera is a section of a sphere, so the corner rays alone do not bound it.  Rays are shot through a
    lattice of 33 x 33 points of the image rectangle [0, W] x [0, H] -- its corners, edge mid-points and centre among them -- and the
    box of their near and far end points is padded by far * delta, where delta = half the diagonal of a lattice cell on the plane at
    unit distance bounds the angle between any pixel's ray and the nearest lattice ray (so far * delta bounds the distance between
    their end points), and then by two cells of a grid of `resolution` vertices per axis."""
    poses = np.asarray(c2w, dtype=np.float64).reshape(-1, *np.shape(c2w)[-2:])[:, :3, :4]
    if not (np.isfinite(near) and np.isfinite(far) and far >= near):
        raise ValueError(f"near {near} far {far}: need finite values with far >= near")
    k = BOUNDS_LATTICE
    u, v = np.meshgrid(np.linspace(0.0, float(width), k), np.linspace(0.0, float(height), k))
    cam = np.stack([(u - cx) / fx, -(v - cy) / fy, -np.ones_like(u)], axis=-1).reshape(-1, 3)
    d = np.einsum("fij,nj->fni", poses[:, :, :3], cam)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = poses[:, None, :, 3]
    pts = np.concatenate([o + near * d, o + far * d], axis=1).reshape(-1, 3)
    delta = 0.5 * float(np.hypot(width / (fx * (k - 1)), height / (fy * (k - 1))))
    lo, hi = pts.min(axis=0) - abs(far) * delta, pts.max(axis=0) + abs(far) * delta
    cell = np.maximum(hi - lo, 1e-6) / max(int(resolution) - 5, 1)  # (res - 1) cells after two more on every side
    return tuple(float(x) for x in (*(lo - 2.0 * cell), *(hi + 2.0 * cell)))


def eval_planes(model) -> Tuple[float, float]:
    """(near, far) the model's collider gives an eval-mode ray bundle that has none of its own."""
    col = getattr(model, "collider", None)
    if col is None:
        p = model.config.collider_params
        return float(p["near_plane"]), float(p["far_plane"])
    near = 0.0 if getattr(col, "reset_near_plane", False) else float(col.near_plane)
    return near, float(col.far_plane)


def attach_occupancy(model, settings: dict, c2w, height: int, width: int, fx: float, fy: float, cx: float, cy: float) -> OccupancyGrid:
    """Build the grid of `settings` ({"resolution", "sigma", "dilate", "bounds"}; bounds None: segment_bounds of the cameras c2w
    with the model's eval planes) from model.field in its current arithmetic and set model.occupancy."""
    res = int(settings.get("resolution", DEFAULT_RESOLUTION))
    bounds = settings.get("bounds")
    if bounds is None:
        near, far = eval_planes(model)
        bounds = segment_bounds(c2w, height, width, fx, fy, cx, cy, near, far, res)
    dev = next(model.field.parameters()).device
    with torch.cuda.device(dev):
        grid = build_occupancy(model.field, bounds, res, float(settings.get("sigma", DEFAULT_SIGMA)),
                               int(settings.get("dilate", DEFAULT_DILATE)))
    model.occupancy = grid
    model.occupancy_samples = bool(settings.get("samples", False))
    return grid


# ------------------------------------------------------------------------------------------------ the two launches
def cull(grid: OccupancyGrid, origins: Tensor, directions: Tensor, nears: Tensor, fars: Tensor) -> Dict[str, Tensor]:
    """rsn_occupancy_cull over R rays (origins / directions fp32 [R,3], nears / fars [R], contiguous, on the grid's device) ->
    hit uint8 [R], n_hit int32 [1] (device), ray_index int32 [R]: the hit rays in ascending order, then the culled ones."""
    lib = _abi.load_library()
    R, dev = int(origins.shape[0]), origins.device
    out = {"hit": torch.empty(R, device=dev, dtype=torch.uint8), "n_hit": torch.empty(1, device=dev, dtype=torch.int32),
           "ray_index": torch.empty(R, device=dev, dtype=torch.int32)}
    ws = torch.empty(max(1, int(lib.rsn_occupancy_cull_workspace_bytes(R)) // 4), device=dev, dtype=torch.int32)
    nx, ny, nz = grid.dims
    check(lib.rsn_occupancy_cull(R, ptr(origins), ptr(directions), ptr(nears), ptr(fars), nx, ny, nz, grid._origin3, grid._spacing3,
                                 ptr(grid.bits), int(grid.outside_occupied), ptr(out["hit"]), ptr(out["n_hit"]), ptr(out["ray_index"]),
                                 ptr(ws), ops._stream()))
    grid.rays_seen += R
    grid.hits_dev += out["n_hit"]
    return out


def scatter_rows(src: Tensor, ray_index: Tensor, n_dev: Optional[Tensor], fill: float) -> Tensor:
    """rsn_scatter_rows: src fp32 [n, ...] (rows of the compacted rays) -> out [n, ...] with out[ray_index[i]] = src[i] for
    i < *n_dev and `fill` in every other row."""
    lib = _abi.load_library()
    n = int(src.shape[0])
    src = ops._f32c(src)
    out = torch.empty_like(src)
    row = src.numel() // n if n else 1
    check(lib.rsn_scatter_rows(n, ptr(n_dev), ptr(ray_index), ptr(src), max(row, 1), float(fill), ptr(out), ops._stream()))
    return out


def mark_and_compact(grid: OccupancyGrid, origins: Tensor, directions: Tensor, pixel_area: Tensor, euclid_bins: Tensor,
                     n_dev: Optional[Tensor] = None, max_radius: Optional[float] = None) -> Dict[str, Tensor]:
    """rsn_occupancy_compact_samples over a level (origins / directions fp32 [R,3], pixel_area [R], euclid_bins [R,S+1], contiguous,
    on the grid's device; n_dev: device int32 count of leading rays, or None) -> live uint8 [R,S], n_live int32 [1] (device),
    sample_index int32 [R*S] (the live samples in ascending order, then the others) and the compact "rays" of one sample each:
    origins_c / directions_c [R*S,3], pixel_area_c [R*S], bins_c [R*S,2], of which the first n_live rows are written.
    max_radius: None = sample_max_radius(grid)."""
    lib = _abi.load_library()
    R, S = int(euclid_bins.shape[0]), int(euclid_bins.shape[1]) - 1
    dev = origins.device
    nbytes = int(lib.rsn_occupancy_samples_workspace_bytes(R, S))
    if nbytes == 0:
        check(-1)
    N = R * S
    f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)  # noqa: E731
    out = {"live": torch.empty(R, S, device=dev, dtype=torch.uint8), "n_live": torch.empty(1, device=dev, dtype=torch.int32),
           "sample_index": torch.empty(N, device=dev, dtype=torch.int32), "origins_c": f(N, 3), "directions_c": f(N, 3),
           "pixel_area_c": f(N), "bins_c": f(N, 2)}
    ws = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
    nx, ny, nz = grid.dims
    radius = sample_max_radius(grid) if max_radius is None else float(max_radius)
    check(lib.rsn_occupancy_compact_samples(R, ptr(n_dev), S, ptr(origins), ptr(directions), ptr(pixel_area), ptr(euclid_bins), nx, ny, nz,
                                            grid._origin3, grid._spacing3, ptr(grid.bits), int(grid.outside_occupied), radius,
                                            ptr(out["live"]), ptr(out["n_live"]), ptr(out["sample_index"]), ptr(out["origins_c"]),
                                            ptr(out["directions_c"]), ptr(out["pixel_area_c"]), ptr(out["bins_c"]), ptr(ws), ops._stream()))
    return out


def scatter_level(compact: Dict[str, Tensor], n_live: Tensor, sample_index: Tensor, lead: Sequence[int]) -> Dict[str, Tensor]:
    """rsn_scatter_level: the members of a level evaluated on the compact samples ([N] or [N,3] each) -> the same keys shaped
    [*lead] / [*lead, 3]: compact row j in slot sample_index[j] for j < *n_live, zeros in the slots of the skipped samples."""
    lib = _abi.load_library()
    N = int(sample_index.shape[0])
    level = {k: torch.empty(*lead, *v.shape[1:], device=v.device, dtype=torch.float32) for k, v in compact.items()}
    src, dst = ops.field_outputs_struct(compact), ops.field_outputs_struct(level)
    check(lib.rsn_scatter_level(N, ptr(n_live), ptr(sample_index), C.byref(src), C.byref(dst), ops._stream()))
    return level


# what a culled ray holds, per output key of the model (everything else: 0)
CULLED_ONE = ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine", "diff")
CULLED_FAR = ("depth_coarse", "depth_fine")


def scatter_outputs(compact: Dict[str, Tensor], culled: Dict[str, Tensor], fars: Tensor) -> Dict[str, Tensor]:
    """Per-ray outputs of the compacted rays ([n, ...] each) -> the same keys in the rays' own order, one rsn_scatter_rows per
    distinct tensor; culled rays get the values of the table in ReflectSamplingNeRFModel._cull.  fars: [n] or [n,1], the rays'
    own order."""
    idx, n_hit = culled["ray_index"], culled["n_hit"]
    done: Dict[tuple, Tensor] = {}
    out = {}
    for k, v in compact.items():
        fill = 1.0 if k in CULLED_ONE else 0.0
        key = (id(v), fill, k in CULLED_FAR)
        if key in done:
            out[k] = done[key]
            continue
        if v.dtype == torch.bool:  # the reflection mask: false for a culled ray
            res = scatter_rows(v.to(torch.float32), idx, n_hit, 0.0) != 0.0
        else:
            res = scatter_rows(v, idx, n_hit, fill)
            if k in CULLED_FAR:
                res = torch.where(culled["hit"].view(-1, *[1] * (res.dim() - 1)) != 0, res, fars.reshape(-1, *[1] * (res.dim() - 1)).to(res.dtype))
        done[key] = out[k] = res
    return out
