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
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _abi, ops
from ._abi import check, ptr

DEFAULT_BOUNDS = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)  # nerfstudio's Blender scene box
DEFAULT_ISO = 10.0  # a starting point, not measured against any scene
DEFAULT_CHUNK = 1 << 18


def _resolution3(resolution: Union[int, Sequence[int]]) -> Tuple[int, int, int]:
    r = (int(resolution),) * 3 if np.ndim(resolution) == 0 else tuple(int(x) for x in resolution)
    if len(r) != 3 or min(r) < 2:
        raise ValueError(f"resolution {resolution!r}: an int or (nx, ny, nz), every entry at least 2")
    return r


def grid_frame(bounds: Sequence[float], resolution: Union[int, Sequence[int]]):
    """-> ((nx, ny, nz), origin [3], spacing [3]) as fp32 numpy: the grid whose first and last vertices sit on `bounds`
    = (x0, y0, z0, x1, y1, z1).  Vertex (i, j, k) is origin + spacing * (i, j, k) in fp32 -- the extractor's arithmetic."""
    n = _resolution3(resolution)
    b = np.asarray(bounds, dtype=np.float64).reshape(6)
    if not (np.all(np.isfinite(b)) and np.all(b[3:] > b[:3])):
        raise ValueError(f"bounds {tuple(bounds)!r}: need x0 y0 z0 x1 y1 z1 with every upper bound above its lower one")
    origin = b[:3].astype(np.float32)
    spacing = ((b[3:] - b[:3]) / (np.asarray(n, dtype=np.float64) - 1.0)).astype(np.float32)
    return n, origin, spacing


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
    o3 = (C.c_float * 3)(*[float(x) for x in origin])
    s3 = (C.c_float * 3)(*[float(x) for x in spacing])
    check(lib.rsn_mesh_emit(nx, ny, nz, ptr(vol), float(iso), o3, s3, ptr(ws), nbytes, n_vert, n_tri,
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


# ------------------------------------------------------------------------------------------------ PLY
PLY_VERTEX_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                             ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("roughness", "<f4"), ("tint_r", "<f4"),
                             ("tint_g", "<f4"), ("tint_b", "<f4")])
PLY_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _np(x, dtype):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def write_ply(path: str, mesh: Dict) -> str:
    """`mesh`: positions [V,3], triangles [T,3], pred_normals [V,3], diff [V,3], roughness [V], tint [V,3] (tensors or arrays)
    -> binary_little_endian 1.0 PLY: per vertex float x y z nx ny nz, uchar red green blue (the diffuse colour,
    floor(clamp(c, 0, 1) * 255 + 0.5)), float roughness tint_r tint_g tint_b; faces as `list uchar int vertex_indices`."""
    pos, tri = _np(mesh["positions"], np.float32).reshape(-1, 3), _np(mesh["triangles"], np.int32).reshape(-1, 3)
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
    face = np.zeros(tri.shape[0], dtype=PLY_FACE_DTYPE)
    face["n"], face["v"] = 3, tri
    kinds = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", "comment reflect_sampling_nerf_amd export-mesh",
              f"element vertex {V}"]
    header += [f"property {kinds[PLY_VERTEX_DTYPE[n].str]} {n}" for n in PLY_VERTEX_DTYPE.names]
    header += [f"element face {tri.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path + ".tmp", "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
    os.replace(path + ".tmp", path)
    return path


# ------------------------------------------------------------------------------------------------ checkpoint -> file
class _Stages:
    """Per-stage device times from events recorded on the current stream: nothing waits until seconds() is read."""

    def __init__(self):
        self.marks = [("start", self._event())]

    @staticmethod
    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def __call__(self, name: str) -> None:
        self.marks.append((name, self._event()))

    def seconds(self) -> Dict[str, float]:
        torch.cuda.synchronize()
        return {name: self.marks[i][1].elapsed_time(e) / 1000.0 for i, (name, e) in enumerate(self.marks[1:])}


def export_mesh(ckpt: str, out: str, resolution: Union[int, Sequence[int]] = 256, bounds: Sequence[float] = DEFAULT_BOUNDS,
                iso: float = DEFAULT_ISO, mma: str = "f32", chunk: int = DEFAULT_CHUNK, device="cuda:0",
                model_config=None) -> dict:
    """Checkpoint (a step-*.ckpt, or a run directory: its newest) -> PLY at `out`.  -> dict with the counts, the grid, iso and
    the seconds per stage (grid evaluation, count, emit, attributes on the device; write on the host)."""
    from .trainer import load_checkpoint, resolve_checkpoint

    ckpt = resolve_checkpoint(ckpt)
    model, step = load_checkpoint(ckpt, model_config, device)
    field = model.field
    field.set_mma_mode(mma)
    (nx, ny, nz), origin, spacing = grid_frame(bounds, resolution)
    with torch.cuda.device(torch.device(device)):
        field.packed_weights()  # the one-off weight packing is not part of the grid stage
        stages = _Stages()
        vol = density_grid(field, bounds, resolution, chunk)
        stages("grid")
        mesh = _extract(vol, iso, origin, spacing, mark=stages)
        mesh.update(vertex_attributes(field, mesh["positions"], spacing, chunk))
        stages("attributes")
        seconds = stages.seconds()
    t0 = time.time()
    write_ply(out, mesh)
    seconds["write"] = time.time() - t0
    return {"checkpoint": ckpt, "step": step, "out": out, "vertices": int(mesh["positions"].shape[0]),
            "triangles": int(mesh["triangles"].shape[0]), "resolution": [nx, ny, nz], "bounds": [float(b) for b in bounds],
            "origin": [float(x) for x in origin], "spacing": [float(x) for x in spacing], "iso": float(iso), "mma": mma,
            "seconds": seconds}
