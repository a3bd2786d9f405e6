"""Export the learnt geometry of a trained field as a coloured triangle mesh (binary PLY), without nerfstudio.

    python -m reflect_sampling_nerf_amd.trainer export-mesh --ckpt FILE|RUN --out mesh.ply [--resolution 256] [--iso 10]

The route: density_grid (the field's sigma at every vertex of a regular grid) -> extract_surface (the iso-surface on the
device: rsn_mesh_count / rsn_mesh_emit of include/rsn.h, marching tetrahedra) -> vertex_attributes (the diffuse colour,
tint, roughness and predicted normal the field holds at each surface vertex: the reference's get_diff, get_tint,
get_roughness, get_pred_normals) -> write_ply.

Every grid or surface point is queried as a Gaussian with variance spacing^2 / 12 per axis -- the footprint of one voxel --
and contracted like the model's samples (field.contract).  The field was trained on integrated encodings: a zero-variance
query lets the 2^16 frequency through and the density turns to noise.

The default iso level (sigma = 10) is a starting point that has not been measured against a scene; so is the default box,
nerfstudio's Blender scene box.  Pick the level per scene.

    ... export-mesh --method tsdf --data DIR | --poses FILE.json [--max-views N] [--downscale K] [--trunc T] [--min-weight 1]

The second route needs no level: fuse_depth takes the model's own median depth (depth_fine, where it starts its reflected rays:
Model.get_surface_outputs) from the given cameras, a few views per launch, off the generator render.surface_maps -- the depth pass
it shares with the point-cloud export -- and fuses the maps into a truncated signed distance volume (rsn_tsdf_integrate of
include/rsn.h) -> tsdf_volume -> the same extractor at level 0 -> drop_unobserved (without it a second shell appears inside
the object, where the observed band ends) -> vertex_attributes -> write_ply.  Its defaults, a truncation of 4 grid spacings and
min_weight 1, are starting points from an experiment on analytic depth maps of a sphere; they have not been measured on a scene.

    ... export-mesh --out mesh.obj --texture [--texels 8] [--min-footprint F]

With --texture either route ends in write_obj of texture.py instead of write_ply: the same four quantities, sampled per texel of a
per-triangle atlas instead of per vertex (texture_atlas -> bake_textures).  Its defaults have not been measured on a scene either.

    ... export-mesh ... [--decimate-cells N | --target-faces N]

With either flag the extracted (and, on the tsdf route, filtered) mesh is reduced by vertex clustering before vertex_attributes
(decimate.py): extract fine, reduce to a budget, let the texture carry the detail.  Without them nothing changes.
"""
from __future__ import annotations

import os
import time
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _abi, ops, render
from ._abi import check, float3, ptr
from ._host import _np, replacing
from .checkpoint import open_checkpoint

DEFAULT_BOUNDS = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)  # nerfstudio's Blender scene box
DEFAULT_ISO = 10.0  # a starting point, not measured against any scene
DEFAULT_CHUNK = 1 << 18


def _frame(bounds: Sequence[float], resolution: Union[int, Sequence[int]], vertices: bool):
    """grid_frame (vertices: n >= 2 per axis, n - 1 intervals between the bounds) and pointcloud.cell_frame (n >= 1 cells, n intervals)."""
    least = 2 if vertices else 1
    n = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(x) for x in resolution)
    if len(n) != 3 or min(n) < least:
        raise ValueError(f"resolution {resolution!r}: an int or (nx, ny, nz), every entry at least {least}")
    b = np.asarray(bounds, dtype=np.float64).reshape(6)
    if not (np.all(np.isfinite(b)) and np.all(b[3:] > b[:3])):
        raise ValueError(f"bounds {tuple(bounds)!r}: need x0 y0 z0 x1 y1 z1 with every upper bound above its lower one")
    intervals = np.asarray(n, dtype=np.float64) - (1.0 if vertices else 0.0)
    return n, b[:3].astype(np.float32), ((b[3:] - b[:3]) / intervals).astype(np.float32)


def grid_frame(bounds: Sequence[float], resolution: Union[int, Sequence[int]]):
    """-> ((nx, ny, nz), origin [3], spacing [3]) as fp32 numpy: the grid whose first and last vertices sit on `bounds`
    = (x0, y0, z0, x1, y1, z1).  Vertex (i, j, k) is origin + spacing * (i, j, k) in fp32 -- the extractor's arithmetic."""
    return _frame(bounds, resolution, vertices=True)


def _voxel_gaussians(field, mean: Tensor, spacing: Tensor):
    """Contracted Gaussians (mean [n,3], cov diagonal [n,3]) of points with one voxel's footprint, as the model contracts."""
    cov = torch.diag_embed((spacing * spacing / 12.0).expand(mean.shape[0], 3))
    m, c = field.contract(mean, cov)
    return m, torch.diagonal(c, dim1=-2, dim2=-1).contiguous()


def density_grid(field, bounds: Sequence[float], resolution: Union[int, Sequence[int]], chunk: int = DEFAULT_CHUNK,
                 mma: Optional[str] = None) -> Tensor:
    """The field's density sigma at every grid vertex -> fp32 [nz, ny, nx] on the field's device.  `mma`: the field's
    matrix-core arithmetic for this and later calls (None: as it stands)."""
    if mma is not None:
        field.set_mma_mode(mma)
    (nx, ny, nz), origin, spacing = grid_frame(bounds, resolution)
    dev = next(field.parameters()).device
    o, s = torch.from_numpy(origin).to(dev), torch.from_numpy(spacing).to(dev)
    n = nx * ny * nz
    vol = torch.empty(n, device=dev, dtype=torch.float32)
    chunk = max(1, int(chunk))
    with torch.no_grad():
        for start in range(0, n, chunk):
            v = torch.arange(start, min(n, start + chunk), device=dev, dtype=torch.int64)
            ijk = torch.stack([v % nx, (v // nx) % ny, v // (nx * ny)], dim=1).to(torch.float32)
            m, cd = _voxel_gaussians(field, o + s * ijk, s)
            vol[start:start + v.numel()] = field.evaluate_gaussians(m, cd, None)["sigma"].reshape(-1)
    return vol.reshape(nz, ny, nx)


def _extract(vol: Tensor, iso: float, origin, spacing, mark=None) -> Dict[str, Tensor]:
    if vol.dim() != 3 or vol.dtype != torch.float32 or vol.device.type != "cuda":
        raise _abi.RsnError("extract_surface: vol must be an fp32 [nz, ny, nx] tensor on a cuda (ROCm) device")
    lib = _abi.load_library()
    vol = vol.contiguous()
    nz, ny, nx = vol.shape
    dev = vol.device
    nbytes = int(lib.rsn_mesh_workspace_bytes(nx, ny, nz))
    if nbytes == 0:
        check(-1)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    check(lib.rsn_mesh_count(nx, ny, nz, ptr(vol), float(iso), ptr(ws), nbytes, ptr(counts), ops._stream()))
    if mark:
        mark("count")
    n_vert, n_tri = (int(x) for x in counts.tolist())  # the one host synchronisation of an export
    pos = torch.empty(n_vert, 3, device=dev, dtype=torch.float32)
    key = torch.empty(n_vert, device=dev, dtype=torch.int32)
    tri = torch.empty(n_tri, 3, device=dev, dtype=torch.int32)
    check(lib.rsn_mesh_emit(nx, ny, nz, ptr(vol), float(iso), float3(origin), float3(spacing), ptr(ws), nbytes, n_vert, n_tri,
                            ptr(pos) if n_vert else None, ptr(key) if n_vert else None, ptr(tri) if n_tri else None,
                            ops._stream()))
    if mark:
        mark("emit")
    return {"positions": pos, "triangles": tri, "vert_key": key}


def extract_surface(vol: Tensor, iso: float, origin: Sequence[float], spacing: Sequence[float]) -> Dict[str, Tensor]:
    """The iso-surface vol == iso of a device volume [nz, ny, nx] (x fastest; vertex (i, j, k) at origin + spacing * (i, j, k)),
    inside = vol >= iso, normals towards lower values -> positions fp32 [V,3], triangles int32 [T,3], vert_key int32 [V]
    (8 * flat grid vertex + edge direction: the grid edge each vertex lies on).  Deterministic: same bits, same order."""
    return _extract(vol, iso, origin, spacing)


def vertex_attributes(field, positions: Tensor, spacing: Sequence[float], chunk: int = DEFAULT_CHUNK) -> Dict[str, Tensor]:
    """What the field predicts at each surface vertex, queried like the grid (one voxel's footprint, contracted, no view
    direction) -> diff [V,3], tint [V,3], roughness [V] (sigmoid), pred_normals [V,3] (unit)."""
    dev = positions.device
    V = positions.shape[0]
    s = torch.as_tensor(np.asarray(spacing, dtype=np.float32), device=dev)
    out = {"diff": torch.empty(V, 3, device=dev), "tint": torch.empty(V, 3, device=dev), "roughness": torch.empty(V, device=dev),
           "pred_normals": torch.empty(V, 3, device=dev)}
    chunk = max(1, int(chunk))
    with torch.no_grad():
        for start in range(0, V, chunk):
            p = positions[start:start + chunk].to(torch.float32)
            m, cd = _voxel_gaussians(field, p, s)
            lv = field.evaluate_gaussians(m, cd, None)
            for k, dst in out.items():
                dst[start:start + p.shape[0]] = lv[k].reshape(dst[start:start + p.shape[0]].shape)
    return out


# ------------------------------------------------------------------------------------------------ TSDF fusion
DEFAULT_TRUNC_SPACINGS = 4.0  # truncation in units of the largest spacing: a starting point from the sphere experiment, not measured on a scene
DEFAULT_MIN_WEIGHT = 1.0      # likewise
DEFAULT_RAY_CHUNK = render.DEFAULT_CHUNK  # rays per chunk of the depth pass
EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # dir 0..6 of vert_key (include/rsn.h)


def integrate_depth(tsdf: Tensor, weight: Tensor, origin, spacing, c2w: Tensor, depth: Tensor, height: int, width: int, fx: float,
                    fy: float, cx: float, cy: float, trunc: float, near: float) -> None:
    """One rsn_tsdf_integrate launch: the views c2w [n,3,4] with depth maps depth [n, H*W] (fp32, on the volumes' device) into
    tsdf / weight (fp32 [nz, ny, nx], contiguous), in place."""
    _abi.check_f32_cuda("integrate_depth", tsdf=tsdf, weight=weight, c2w=c2w, depth=depth)
    if tsdf.dim() != 3 or weight.shape != tsdf.shape:
        raise _abi.RsnError("integrate_depth: tsdf and weight must be [nz, ny, nx] tensors of one shape")
    n = int(c2w.shape[0])
    if tuple(c2w.shape) != (n, 3, 4) or depth.numel() != n * int(height) * int(width):
        raise _abi.RsnError(f"integrate_depth: c2w {tuple(c2w.shape)} / depth {tuple(depth.shape)}: need [n,3,4] and [n, {height}*{width}]")
    nz, ny, nx = tsdf.shape
    check(_abi.load_library().rsn_tsdf_integrate(nx, ny, nz, float3(origin), float3(spacing), n, ptr(c2w), int(height), int(width),
                                                 float(fx), float(fy), float(cx), float(cy), ptr(depth), float(trunc), float(near),
                                                 ptr(tsdf), ptr(weight), ops._stream()))


def fuse_depth(model, poses, H: int, W: int, fx: float, fy: float, cx: float, cy: float, bounds: Sequence[float],
               resolution: Union[int, Sequence[int]], trunc: float, views_per_launch: int = 8, chunk: int = DEFAULT_RAY_CHUNK,
               events: Optional[list] = None) -> Tuple[Tensor, Tensor]:
    """Render the model's median depth (Model.get_surface_outputs: depth_fine) from the cameras poses [F,3,4] (or [F,4,4]) with
    one pinhole H x W, fx, fy, cx, cy, and fuse the maps into the grid of grid_frame(bounds, resolution) -> (tsdf, weight), fp32
    [nz, ny, nx] on the model's device, both starting at zero.  `near` of the fusion is the model's collider near plane.
    views_per_launch depth maps are held at a time and go into one rsn_tsdf_integrate launch (the result does not depend on it);
    chunk: rays per chunk of the depth pass.  No device-to-host read.
    events: a list that receives, per launch, three timing events: start, depth maps rendered, integrated."""
    (nx, ny, nz), origin, spacing = grid_frame(bounds, resolution)
    dev = model.device
    near = float(model.config.collider_params["near_plane"])
    tsdf = torch.zeros(nz, ny, nx, device=dev, dtype=torch.float32)
    weight = torch.zeros(nz, ny, nx, device=dev, dtype=torch.float32)
    with torch.no_grad():
        for _, c2w, depth, _ in render.surface_maps(model, poses, H, W, fx, fy, cx, cy, views_per_launch, chunk, events=events):
            integrate_depth(tsdf, weight, origin, spacing, c2w, depth, H, W, fx, fy, cx, cy, trunc, near)
            ops.record_event(events and events[-1])
    return tsdf, weight


def tsdf_volume(tsdf: Tensor, weight: Tensor, min_weight: float = DEFAULT_MIN_WEIGHT) -> Tensor:
    """The volume the extractor takes at level 0: -tsdf where weight >= min_weight, else -1.  The extractor's "inside = vol >= 0"
    then means "behind the surface", and a vertex no view reached counts as outside."""
    return torch.where(weight >= min_weight, -tsdf, torch.full_like(tsdf, -1.0))


def drop_unobserved(mesh: Dict[str, Tensor], weight: Tensor, dims: Sequence[int], min_weight: float = DEFAULT_MIN_WEIGHT) -> Dict[str, Tensor]:
    """Keep the part of an extracted mesh that lies between observed grid vertices.  A surface vertex sits on the grid edge its
    vert_key = 8 v + dir names; it is valid if and only if both ends of that edge have weight >= min_weight.  The triangles whose
    three vertices are valid stay, in their order; the vertices no remaining triangle names are dropped and the others renumbered
    in their order.  dims = (nx, ny, nz) of weight [nz, ny, nx].  Plain torch operations: CPU tensors work as well.
    -> {"positions", "triangles", "vert_key"} (and every other per-vertex entry of `mesh`, filtered alike)."""
    nx, ny, _ = (int(d) for d in dims)
    key = mesh["vert_key"].to(torch.int64)
    tri = mesh["triangles"].to(torch.int64).reshape(-1, 3)
    V = key.shape[0]
    off = torch.tensor([dx + dy * nx + dz * nx * ny for dx, dy, dz in EDGE_OFFSETS] + [0], device=key.device, dtype=torch.int64)
    lo = torch.div(key, 8, rounding_mode="floor")
    seen = weight.reshape(-1) >= min_weight
    valid = seen[lo] & seen[lo + off[key % 8]]
    tri = tri[valid[tri].all(dim=1)]
    used = torch.zeros(V, device=key.device, dtype=torch.bool)
    used[tri.reshape(-1)] = True
    new_id = torch.cumsum(used.to(torch.int64), dim=0) - 1
    out = {k: v[used] for k, v in mesh.items() if k != "triangles" and isinstance(v, Tensor) and v.shape[:1] == (V,)}
    out["triangles"] = new_id[tri].to(mesh["triangles"].dtype)
    return out


# ------------------------------------------------------------------------------------------------ PLY
PLY_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                             ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("roughness", "<f4"), ("tint_r", "<f4"),
                             ("tint_g", "<f4"), ("tint_b", "<f4")])
PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path: str, mesh: Dict) -> str:
    """`mesh`: positions [V,3], triangles [T,3], pred_normals [V,3], diff [V,3], roughness [V], tint [V,3] (tensors or arrays)
    -> binary_little_endian 1.0 PLY: per vertex float x y z nx ny nz, uchar red green blue (the diffuse colour,
    floor(clamp(c, 0, 1) * 255 + 0.5)), float roughness tint_r tint_g tint_b; faces as `list uchar int vertex_indices`."""
    return _write_ply(path, mesh, "export-mesh", faces=True)


def _write_ply(path: str, mesh: Dict, command: str, faces: bool) -> str:
    """The PLY of write_ply (faces) and of pointcloud.write_ply_points (the vertex element alone); `command` ends the comment line."""
    pos = _np(mesh["positions"], np.float32).reshape(-1, 3)
    V = pos.shape[0]
    vert = np.zeros(V, dtype=PLY_VERTEX_DTYPE)
    nrm = _np(mesh["pred_normals"], np.float32).reshape(V, 3)
    rgb = np.floor(np.clip(_np(mesh["diff"], np.float32).reshape(V, 3), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    tint = _np(mesh["tint"], np.float32).reshape(V, 3)
    for c, (p, q) in enumerate((("x", "nx"), ("y", "ny"), ("z", "nz"))):
        vert[p], vert[q] = pos[:, c], nrm[:, c]
    for c, name in enumerate(("red", "green", "blue")):
        vert[name] = rgb[:, c]
    vert["roughness"] = _np(mesh["roughness"], np.float32).reshape(V)
    for c, name in enumerate(("tint_r", "tint_g", "tint_b")):
        vert[name] = tint[:, c]
    kinds = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"comment reflect_sampling_nerf_amd {command}", f"element vertex {V}"]
    header += [f"property {kinds[PLY_VERTEX_DTYPE[n].str]} {n}" for n in PLY_VERTEX_DTYPE.names]
    face = np.zeros(0, dtype=PLY_FACE_DTYPE)
    if faces:
        tri = _np(mesh["triangles"], np.int32).reshape(-1, 3)
        face = np.zeros(tri.shape[0], dtype=PLY_FACE_DTYPE)
        face["n"], face["v"] = 3, tri
        header += [f"element face {tri.shape[0]}", "property list uchar int vertex_indices"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with replacing(path) as tmp, open(tmp, "wb") as fh:
        fh.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
    return path


# ------------------------------------------------------------------------------------------------ checkpoint -> file
class _Stages:
    """Per-stage device times from events recorded on the current stream: nothing waits until seconds() is read."""

    def __init__(self):
        self.names, self.events = [], []
        ops.record_event(self.events)  # the start of the first stage

    def __call__(self, name: str) -> None:
        self.names.append(name)
        ops.record_event(self.events)

    def seconds(self) -> Dict[str, float]:
        torch.cuda.synchronize()
        return {name: a.elapsed_time(b) / 1000.0 for name, a, b in zip(self.names, self.events, self.events[1:])}


def export_mesh(ckpt: str, out: str, resolution: Union[int, Sequence[int]] = 256, bounds: Sequence[float] = DEFAULT_BOUNDS,
                iso: float = DEFAULT_ISO, mma: str = "f32", chunk: int = DEFAULT_CHUNK, device="cuda:0",
                model_config=None, method: str = "density", cameras: Optional[dict] = None, trunc: Optional[float] = None,
                min_weight: float = DEFAULT_MIN_WEIGHT, views_per_launch: int = 8, ray_chunk: int = DEFAULT_RAY_CHUNK,
                texture: bool = False, texels: int = 8, min_footprint: Optional[float] = None,
                decimate_cells: Optional[int] = None, target_faces: Optional[int] = None) -> dict:
    """Checkpoint (a step-*.ckpt, or a run directory: its newest) -> PLY at `out` (texture=True: a textured OBJ, see below).  -> dict with the counts, the grid, the method
    and the seconds per stage.
    method "density": the iso-surface of the field's density at `iso`; stages: grid evaluation, count, emit, attributes on the
    device; write on the host.
    method "tsdf": the surface of the model's own depth maps (see the module text); `iso` plays no part.  cameras: {"c2w" [F,3,4],
    "width", "height", "fx", "fy", "cx", "cy"} (what trainer.resolve_export_cameras returns); trunc: the truncation distance in
    world units (None: DEFAULT_TRUNC_SPACINGS x the largest spacing); min_weight: the views a grid vertex needs to count as
    observed.  Stages: depth (the depth passes), integrate, count, emit, filter, attributes; write.  The dict also holds the view
    count, trunc, min_weight and the counts before the filter.
    texture=True (either method): `out` must end in .obj and becomes a textured OBJ with its MTL and four PNG maps beside it
    (texture.py) instead of a PLY; texels: the side of the square of texels a pair of triangles gets; min_footprint: the smallest
    footprint a texel is queried with (None: the largest spacing / 8) -- both defaults are starting points, not measured on a
    scene.  The stages atlas and bake join the seconds, texture_size, texels, live_texels, min_footprint and files the dict.
    decimate_cells=N or target_faces=N (one of them at most; either method, with or without texture): the extracted mesh -- on the
    tsdf route after its filter, which needs vert_key -- is reduced by vertex clustering before anything else sees it (decimate.py):
    with N cluster cells per axis over `bounds`, or with the cell count decimate_to finds for at most N triangles, looking from 2 up
    to the grid's intervals per axis (finer clusters than the grid merge nothing).  The attributes of the merged vertices are then
    queried with the CLUSTER CELL as `spacing` of vertex_attributes -- a merged vertex stands for a cell; a design rule that has not
    been measured against a scene.  The texture bake is unchanged: it sees a mesh.  The dict gains vertices_extracted /
    triangles_extracted (where the tsdf route has not set them), `decimate` (decimate.py's stats) and the stage decimate."""
    decimating = decimate_cells is not None or target_faces is not None
    if decimating:
        from . import decimate as dec

        if decimate_cells is not None and target_faces is not None:
            raise ValueError("decimate_cells and target_faces exclude each other")
        if (decimate_cells if target_faces is None else target_faces) < 1:
            raise ValueError(f"decimate_cells {decimate_cells} / target_faces {target_faces}: need a value of at least 1")
    if texture:
        from . import texture as tex

        tex.obj_file_set(out)    # the argument errors come before the checkpoint is read
        tex.atlas_shape(0, texels)
        footprint_lo, _ = tex.footprint_bounds(grid_frame(bounds, resolution)[2], min_footprint)

    if method not in ("density", "tsdf"):
        raise ValueError(f"method {method!r}: density or tsdf")
    if method == "tsdf" and cameras is None:
        raise ValueError("method tsdf needs cameras")
    ckpt, model, step = open_checkpoint(ckpt, model_config, device, mma)
    field = model.field
    (nx, ny, nz), origin, spacing = grid_frame(bounds, resolution)
    extra = {}
    with torch.cuda.device(torch.device(device)):
        field.packed_weights()  # the one-off weight packing is not part of the grid stage
        stages = _Stages()
        if method == "density":
            vol = density_grid(field, bounds, resolution, chunk)
            stages("grid")
            mesh = _extract(vol, iso, origin, spacing, mark=stages)
        else:
            trunc = float(DEFAULT_TRUNC_SPACINGS * float(spacing.max()) if trunc is None else trunc)
            events: list = []
            tsdf, weight = fuse_depth(model, *render.camera_args(cameras), bounds, resolution, trunc, views_per_launch, ray_chunk, events)
            vol = tsdf_volume(tsdf, weight, min_weight)
            stages("fuse")
            mesh = _extract(vol, 0.0, origin, spacing, mark=stages)
            extra = {"views": int(len(cameras["c2w"])), "trunc": trunc, "min_weight": float(min_weight),
                     "vertices_extracted": int(mesh["positions"].shape[0]), "triangles_extracted": int(mesh["triangles"].shape[0]),
                     "image": [int(cameras["width"]), int(cameras["height"])]}
            mesh = drop_unobserved(mesh, weight, (nx, ny, nz), min_weight)
            stages("filter")
        attribute_spacing = spacing
        if decimating:
            extra.setdefault("vertices_extracted", int(mesh["positions"].shape[0]))
            extra.setdefault("triangles_extracted", int(mesh["triangles"].shape[0]))
            if target_faces is not None:
                mesh, extra["decimate"] = dec.decimate_to(mesh, bounds, target_faces, max(2, max(nx, ny, nz) - 1))
            else:
                mesh = dec.decimate(mesh, bounds, decimate_cells)
                extra["decimate"] = mesh.pop("stats")
            attribute_spacing = np.asarray(extra["decimate"]["cell_size"], dtype=np.float32)
            stages("decimate")
        mesh.update(vertex_attributes(field, mesh["positions"], attribute_spacing, chunk))
        stages("attributes")
        if texture:
            attributes = tex.field_attributes(field, spacing, footprint_lo, chunk)
            atlas = tex.texture_atlas(mesh["positions"], mesh["triangles"], texels)
            stages("atlas")
            maps = tex.bake_textures(attributes, atlas, chunk)
            stages("bake")
            extra.update(texture_size=int(atlas["size"]), texels=int(texels), live_texels=int(atlas["live"].numel()),
                         min_footprint=footprint_lo)
        seconds = stages.seconds()
        if method == "tsdf":  # the fuse stage, split into its two kinds of work by the per-launch events
            del seconds["fuse"]
            seconds = {"depth": sum(e[0].elapsed_time(e[1]) for e in events) / 1000.0,
                       "integrate": sum(e[1].elapsed_time(e[2]) for e in events) / 1000.0, **seconds}
            extra["integrate_launches"] = len(events)
    t0 = time.time()
    if texture:
        extra["files"] = tex.write_obj(out, mesh, atlas["uv"], maps)
    else:
        write_ply(out, mesh)
    seconds["write"] = time.time() - t0
    res = {"checkpoint": ckpt, "step": step, "out": out, "vertices": int(mesh["positions"].shape[0]),
           "triangles": int(mesh["triangles"].shape[0]), "resolution": [nx, ny, nz], "bounds": [float(b) for b in bounds],
           "origin": [float(x) for x in origin], "spacing": [float(x) for x in spacing], "method": method, "mma": mma,
           "seconds": seconds}
    if method == "density":
        res["iso"] = float(iso)
    res.update(extra)
    return res
