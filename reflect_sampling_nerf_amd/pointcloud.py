"""Export the surface a trained model renders as a coloured point cloud (binary PLY without faces), without nerfstudio.

    python -m reflect_sampling_nerf_amd.trainer export-pointcloud --ckpt FILE|RUN --out cloud.ply --data DIR | --poses FILE.json
        [--max-views N] [--downscale K] [--resolution 512] [--min-accumulation 0.5] [--edge 0.05 | --no-edge] [--no-thin]

A point is exactly where the model starts a reflected ray: origin + depth_fine * direction of a pixel.  No grid resampling, iso
level or truncation distance comes between the model and the file.  The route: collect_points takes the model's median depth
and accumulation from the given cameras (Model.get_surface_outputs: the depth-only pass) off the generator render.surface_maps,
the depth pass it shares with the TSDF route of export-mesh, and rsn_pointcloud_mark /
rsn_pointcloud_select of include/rsn.h turn the maps into one set of points -- a pixel is a candidate when its depth is finite
and positive, its accumulation reaches `min_accumulation`, its depth differs from no neighbour's by more than `edge` times the
smaller of the two (silhouette pixels go) and its point lies in `bounds`; with thinning, a grid of resolution^3 cells over the
bounds keeps one point per cell, the candidate with the lowest global pixel index -> mesh.vertex_attributes (the diffuse colour,
tint, roughness and predicted normal the field holds at each point, queried with one cell's footprint) -> write_ply_points.

The order of the points is that of their global pixel index ((view*H + y)*W + x): two runs give identical bytes, whatever the
number of views per launch.

The colour of a point is the field's DIFFUSE colour at the point, not a rendered pixel: it holds no reflection and does not depend
on a viewing direction.  The defaults -- 512 cells per axis, accumulation 0.5, edge 0.05 -- are starting points that have not been
measured on a scene.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Dict, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _abi, mesh, ops, render
from ._abi import check, float3, ptr
from .checkpoint import open_checkpoint

DEFAULT_RESOLUTION = 512       # cells per axis of the thinning grid: a starting point, not measured on a scene
DEFAULT_MIN_ACCUMULATION = 0.5  # likewise
DEFAULT_EDGE = 0.05            # likewise; math.inf switches the depth-edge test off
NO_OWNER = 0x7FFFFFFF          # what an owner array holds before the first mark


def cell_frame(bounds: Sequence[float], resolution: Union[int, Sequence[int]]):
    """-> ((nx, ny, nz), origin [3], spacing [3]) as fp32 numpy: the grid of nx * ny * nz CELLS that tiles `bounds` =
    (x0, y0, z0, x1, y1, z1); cell (i, j, k) spans origin + spacing * (i..i+1, j..j+1, k..k+1)."""
    return mesh._frame(bounds, resolution, vertices=False)


def new_owner(dims: Sequence[int], device) -> Tensor:
    """The owner array of a grid of dims = (nx, ny, nz) cells, int32 [nz, ny, nx] on `device`, with no cell taken."""
    nx, ny, nz = (int(d) for d in dims)
    return torch.full((nz, ny, nx), NO_OWNER, device=device, dtype=torch.int32)


def _views(who, c2w, depth, accumulation, height, width):
    n = int(c2w.shape[0])
    _abi.check_f32_cuda(who, c2w=c2w, depth=depth, accumulation=accumulation)
    if tuple(c2w.shape) != (n, 3, 4) or depth.numel() != n * int(height) * int(width) or (
            accumulation is not None and accumulation.numel() != depth.numel()):
        raise _abi.RsnError(f"{who}: c2w {tuple(c2w.shape)} / depth {tuple(depth.shape)}: need [n,3,4] and [n, {height}*{width}] "
                            "(accumulation like depth)")
    return n


def _grid_args(dims, origin, spacing, owner):
    nx, ny, nz = (int(d) for d in dims)
    if owner is not None and (owner.dtype != torch.int32 or owner.device.type != "cuda" or not owner.is_contiguous()
                              or tuple(owner.shape) != (nz, ny, nx)):
        raise _abi.RsnError(f"owner must be a contiguous int32 [{nz}, {ny}, {nx}] tensor on a cuda (ROCm) device")
    return nx, ny, nz, float3(origin), float3(spacing)


def mark(owner: Optional[Tensor], dims, origin, spacing, c2w: Tensor, depth: Tensor, accumulation: Optional[Tensor], height: int,
         width: int, fx: float, fy: float, cx: float, cy: float, view0: int, min_accumulation: float, edge: float) -> None:
    """One rsn_pointcloud_mark launch: the candidates of the views c2w [n,3,4] with depth / accumulation [n, H*W] (fp32, device;
    accumulation may be None) claim their cells in owner (int32 [nz, ny, nx], in place; None: no thinning, nothing is launched)."""
    n = _views("pointcloud.mark", c2w, depth, accumulation, height, width)
    nx, ny, nz, o3, s3 = _grid_args(dims, origin, spacing, owner)
    check(_abi.load_library().rsn_pointcloud_mark(n, ptr(c2w), int(height), int(width), float(fx), float(fy), float(cx), float(cy),
                                                  ptr(depth), ptr(accumulation), int(view0), nx, ny, nz, o3, s3,
                                                  float(min_accumulation), float(edge), ptr(owner), ops._stream()))


def select(owner: Optional[Tensor], dims, origin, spacing, c2w: Tensor, depth: Tensor, accumulation: Optional[Tensor], height: int,
           width: int, fx: float, fy: float, cx: float, cy: float, view0: int, min_accumulation: float, edge: float,
           out: Optional[Tuple[Tensor, Tensor, Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """One rsn_pointcloud_select call -> (counts int32 [2] = (kept rows, candidates before the owner test), pixel_index int32
    [n*H*W], positions fp32 [n*H*W, 3]) on the device; rows at and past the count are not written.  out: (counts, pixel_index,
    positions, workspace uint8) to write into instead of fresh tensors, each at least as large.  No device-to-host read."""
    n = _views("pointcloud.select", c2w, depth, accumulation, height, width)
    nx, ny, nz, o3, s3 = _grid_args(dims, origin, spacing, owner)
    lib = _abi.load_library()
    dev = depth.device
    rows = n * int(height) * int(width)
    nbytes = int(lib.rsn_pointcloud_workspace_bytes(n, int(height), int(width)))
    if nbytes == 0:
        check(-1)
    if out is None:
        out = (torch.empty(2, device=dev, dtype=torch.int32), torch.empty(rows, device=dev, dtype=torch.int32),
               torch.empty(rows, 3, device=dev, dtype=torch.float32), torch.empty(nbytes, device=dev, dtype=torch.uint8))
    counts, pixel_index, positions, ws = out
    if counts.numel() < 2 or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise _abi.RsnError("pointcloud.select: counts must be a contiguous int32 tensor of two entries")
    if pixel_index.numel() < rows or positions.numel() < 3 * rows or ws.numel() < nbytes:
        raise _abi.RsnError(f"pointcloud.select: the output buffers hold fewer than {rows} rows or the workspace fewer than {nbytes} bytes")
    check(lib.rsn_pointcloud_select(n, ptr(c2w), int(height), int(width), float(fx), float(fy), float(cx), float(cy), ptr(depth),
                                    ptr(accumulation), int(view0), nx, ny, nz, o3, s3, float(min_accumulation), float(edge),
                                    ptr(owner), ptr(ws), ws.numel(), ptr(counts), C.c_void_p(counts.data_ptr() + 4), ptr(pixel_index),
                                    ptr(positions), ops._stream()))
    return counts, pixel_index, positions


def collect_points(model, poses, H: int, W: int, fx: float, fy: float, cx: float, cy: float, bounds: Sequence[float],
                   resolution: Union[int, Sequence[int]], min_accumulation: float, edge: float, thin: bool = True,
                   views_per_launch: int = 8, chunk: int = mesh.DEFAULT_RAY_CHUNK, events: Optional[list] = None) -> Dict[str, Tensor]:
    """Render the model's median depth and accumulation (Model.get_surface_outputs: depth_fine, accumulation_fine) from the
    cameras poses [F,3,4] (or [F,4,4]) with one pinhole H x W, fx, fy, cx, cy, views_per_launch views at a time, and keep the
    candidate pixels' points (the rule: module text and include/rsn.h) -- with `thin` one per cell of cell_frame(bounds,
    resolution), without it all of them (the grid then only bounds the cloud) -> {"positions" fp32 [P,3], "pixel_index" int32 [P]
    (the global pixel index (view*H + y)*W + x, ascending)} on the model's device, and "candidates": the number of candidates
    before thinning (an int).  The result does not depend on views_per_launch or chunk (rays per chunk of the depth pass).

    One device-to-host read per launch: the two counts of the selection (kept rows, which size the slice that is kept, and
    candidates) in one copy.  Nothing else is read back.
    events: a list that receives, per launch, four timing events: start, maps rendered, marked, selected."""
    dims, origin, spacing = cell_frame(bounds, resolution)
    F, H, W = len(poses), int(H), int(W)
    dev = model.device
    if F * H * W > 2 ** 31 - 1:
        raise ValueError(f"{F} views of {W} x {H} pixels: the global pixel index needs views * H * W <= 2^31 - 1")
    owner = new_owner(dims, dev) if thin else None
    per = min(max(1, int(views_per_launch)), max(F, 1))  # the views of the largest launch: what the selection's buffers hold
    nbytes = int(_abi.load_library().rsn_pointcloud_workspace_bytes(per, H, W))
    if nbytes == 0:
        check(-1)
    out = (torch.empty(2, device=dev, dtype=torch.int32), torch.empty(per * H * W, device=dev, dtype=torch.int32),
           torch.empty(per * H * W, 3, device=dev, dtype=torch.float32), torch.empty(nbytes, device=dev, dtype=torch.uint8))
    candidates = 0
    index, points = [], []
    with torch.no_grad():
        for start, c2w, depth, acc in render.surface_maps(model, poses, H, W, fx, fy, cx, cy, views_per_launch, chunk, True, events):
            views = (dims, origin, spacing, c2w, depth, acc, H, W, fx, fy, cx, cy, start, min_accumulation, edge)
            mark(owner, *views)
            ops.record_event(events and events[-1])
            counts, pixel_index, positions = select(owner, *views, out=out)
            ops.record_event(events and events[-1])
            kept, cand = (int(x) for x in counts.tolist())  # the one read of the launch
            candidates += cand
            index.append(pixel_index[:kept].clone())
            points.append(positions[:kept].clone())
    return {"positions": torch.cat(points) if points else torch.empty(0, 3, device=dev, dtype=torch.float32),
            "pixel_index": torch.cat(index) if index else torch.empty(0, device=dev, dtype=torch.int32), "candidates": candidates}


# ------------------------------------------------------------------------------------------------ PLY
def write_ply_points(path: str, cloud: Dict) -> str:
    """`cloud`: positions [P,3], pred_normals [P,3], diff [P,3], roughness [P], tint [P,3] (tensors or arrays) ->
    binary_little_endian 1.0 PLY with one element, vertex, in the layout of mesh.write_ply (mesh.PLY_VERTEX_DTYPE): float x y z
    nx ny nz (the predicted normal), uchar red green blue (the field's diffuse colour, floor(clamp(c, 0, 1) * 255 + 0.5)), float
    roughness tint_r tint_g tint_b.  There is no face element.  Written to a temporary file that is then renamed."""
    return mesh._write_ply(path, cloud, "export-pointcloud", faces=False)


# ------------------------------------------------------------------------------------------------ checkpoint -> file
def export_pointcloud(ckpt: str, out: str, cameras: dict, resolution: Union[int, Sequence[int]] = DEFAULT_RESOLUTION,
                      bounds: Sequence[float] = mesh.DEFAULT_BOUNDS, min_accumulation: float = DEFAULT_MIN_ACCUMULATION,
                      edge: float = DEFAULT_EDGE, thin: bool = True, mma: str = "f32", ray_chunk: int = mesh.DEFAULT_RAY_CHUNK,
                      chunk: int = mesh.DEFAULT_CHUNK, views_per_launch: int = 8, device="cuda:0", model_config=None) -> dict:
    """Checkpoint (a step-*.ckpt, or a run directory: its newest) -> PLY point cloud at `out`.  cameras: {"c2w" [F,3,4], "width",
    "height", "fx", "fy", "cx", "cy"} (what trainer.resolve_export_cameras returns); edge: math.inf switches the depth-edge test
    off; ray_chunk: rays per chunk of the depth pass; chunk: points per field launch of the attribute pass.  -> dict: checkpoint,
    step, out, points, candidates (before thinning), views, image [W, H], resolution (cells per axis), bounds, spacing,
    min_accumulation, edge, thin, mma and seconds = {depth, mark, select, attributes} on the device, from events, and write on the
    host."""
    if min_accumulation != min_accumulation or not edge >= 0.0:
        raise ValueError(f"min_accumulation {min_accumulation} / edge {edge}: need a number and an edge >= 0 (inf: no edge test)")
    ckpt, model, step = open_checkpoint(ckpt, model_config, device, mma)
    field = model.field
    dims, _, spacing = cell_frame(bounds, resolution)
    with torch.cuda.device(torch.device(device)):
        field.packed_weights()  # the one-off weight packing is not part of the depth stage
        events: list = []
        cloud = collect_points(model, *render.camera_args(cameras), bounds, resolution, min_accumulation, edge, thin, views_per_launch,
                               ray_chunk, events)
        stages = mesh._Stages()
        cloud.update(mesh.vertex_attributes(field, cloud["positions"], spacing, chunk))
        stages("attributes")
        seconds = stages.seconds()
        seconds = {"depth": sum(e[0].elapsed_time(e[1]) for e in events) / 1000.0,
                   "mark": sum(e[1].elapsed_time(e[2]) for e in events) / 1000.0,
                   "select": sum(e[2].elapsed_time(e[3]) for e in events) / 1000.0, **seconds}
        candidates = int(cloud.pop("candidates"))
    t0 = time.time()
    write_ply_points(out, cloud)
    seconds["write"] = time.time() - t0
    return {"checkpoint": ckpt, "step": step, "out": out, "points": int(cloud["positions"].shape[0]), "candidates": candidates,
            "views": int(len(cameras["c2w"])), "image": [int(cameras["width"]), int(cameras["height"])], "resolution": list(dims),
            "bounds": [float(b) for b in bounds], "spacing": [float(x) for x in spacing], "min_accumulation": float(min_accumulation),
            "edge": float(edge), "thin": bool(thin), "mma": mma, "seconds": seconds}
