"""Textured mesh export: the field's material maps baked into a per-triangle atlas (OBJ + MTL + four PNG maps).

    python -m reflect_sampling_nerf_amd.trainer export-mesh --ckpt FILE|RUN --out mesh.obj --texture [--texels 8] [--min-footprint F]

The PLY of export-mesh carries diffuse colour, tint, roughness and predicted normal per vertex, so the material is as coarse as the
geometry.  Here every pair of triangles owns one square of texels x texels texels of an N x N atlas (the layout: include/rsn.h,
"texture atlas"), and the field is queried once per live texel: texture_atlas (rsn_texture_points: the point on the triangle and
the footprint of every texel) -> bake_textures (the attributes at the live texels, scattered and quantised by rsn_visualize) ->
write_obj.  The maps are the field's material decomposition -- diffuse colour, tint, roughness, predicted normal --, not a rendered
colour: a rendered colour holds the reflections of one viewpoint.

A texel is queried as an isotropic Gaussian of variance f^2 / 12 with f = clamp(footprint, min_footprint, largest grid spacing):
never blurrier than a per-vertex sample, and never so sharp that a sliver triangle lets the top encoding frequencies through (see
the module text of mesh.py).  The defaults, 8 texels per square side and min_footprint = largest spacing / 8, are starting points
that have not been measured on a scene.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from . import _abi, ops
from ._abi import RSN_VIS_GRAY, RSN_VIS_RGB, RSN_VIS_UNIT, check, ptr
from ._host import _np, replacing
from .render import visualize

DEFAULT_TEXELS = 8            # texels per square side: a starting point, not measured on a scene
MIN_FOOTPRINT_FRACTION = 8.0  # default min_footprint = largest spacing / 8: a starting point, not measured on a scene
MAX_SIZE = 16384              # the limit of rsn_texture_points
DEFAULT_CHUNK = 1 << 18
MAPS = ("diffuse", "tint", "roughness", "normal")  # the file NAME_<map>.png of each
MTL_KEYS = (("map_Kd", "diffuse"), ("map_Ks", "tint"), ("map_Pr", "roughness"), ("norm", "normal"))
_ROWS_PER_FORMAT = 1 << 16    # text rows formatted at a time


def atlas_shape(n_triangles: int, texels: int = DEFAULT_TEXELS):
    """-> (squares_per_row Q, size N) of the atlas of n_triangles triangles: S = ceil(T / 2) squares, Q = max(1, ceil(sqrt(S))) in
    integers, N = Q * texels.  ValueError for texels < 4 and for N > 16384."""
    T, P = int(n_triangles), int(texels)
    if P < 4:
        raise ValueError(f"texels {texels}: a square needs at least 4 x 4 texels (--texels)")
    if T < 0:
        raise ValueError(f"n_triangles {n_triangles}: need a count >= 0")
    S = (T + 1) // 2
    Q = int(np.sqrt(float(S)))
    while Q * Q < S:
        Q += 1
    while Q > 1 and (Q - 1) * (Q - 1) >= S:
        Q -= 1
    Q = max(1, Q)
    N = Q * P
    if N > MAX_SIZE:
        raise ValueError(f"{T} triangles at {P} texels per square side need an atlas of {N} x {N} texels, more than {MAX_SIZE}: "
                         "lower --texels, or --resolution for fewer triangles")
    return Q, N


def atlas_uv(n_triangles: int, texels: int, squares_per_row: int) -> np.ndarray:
    """The OBJ texture coordinates of every triangle's corners -> float64 [T,3,2]: corner k at texel centre (col_k, row_k) has
    vt = ((col_k + 0.5) / N, 1 - (row_k + 0.5) / N), image row 0 at the top."""
    T, P, Q = int(n_triangles), int(texels), int(squares_per_row)
    N = Q * P
    t = np.arange(T, dtype=np.int64)
    q, upper = t // 2, (t % 2).astype(bool)
    corner = np.where(upper[:, None, None], np.array([[P - 1, P - 1], [2, P - 1], [P - 1, 2]], dtype=np.int64),
                      np.array([[0, 0], [P - 3, 0], [0, P - 3]], dtype=np.int64))  # (a, b) = (column, row) inside the square
    col = (q % Q)[:, None] * P + corner[:, :, 0]
    row = (q // Q)[:, None] * P + corner[:, :, 1]
    return np.stack([(col + 0.5) / N, 1.0 - (row + 0.5) / N], axis=-1).reshape(T, 3, 2)


def texture_atlas(positions: Tensor, triangles: Tensor, texels: int = DEFAULT_TEXELS) -> Dict:
    """The atlas of a device mesh (positions fp32 [V,3], triangles int32 [T,3]) -> {"size" N, "squares_per_row", "texels", "face"
    int32 [N,N] (the triangle a texel samples, -1: unused), "point" fp32 [N,N,3], "footprint" fp32 [N,N], "live" int64 [n] (the flat
    indices of the used texels, ascending), "uv" float64 [T,3,2] (numpy)}.  One rsn_texture_points launch; reading `live` waits for
    it.  texels: 8 is a starting point, not measured on a scene."""
    if positions.device.type != "cuda" or triangles.device != positions.device:
        raise _abi.RsnError("texture_atlas: positions and triangles must be on one cuda (ROCm) device")
    T = int(triangles.shape[0])
    Q, N = atlas_shape(T, texels)
    dev = positions.device
    pos = positions.to(torch.float32).reshape(-1, 3).contiguous()
    tri = triangles.to(torch.int32).reshape(-1, 3).contiguous()
    if T:
        face = torch.empty(N, N, device=dev, dtype=torch.int32)
        point = torch.empty(N, N, 3, device=dev, dtype=torch.float32)
        footprint = torch.empty(N, N, device=dev, dtype=torch.float32)
    else:  # the call launches nothing: every texel is unused
        face = torch.full((N, N), -1, device=dev, dtype=torch.int32)
        point = torch.zeros(N, N, 3, device=dev, dtype=torch.float32)
        footprint = torch.zeros(N, N, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        check(_abi.load_library().rsn_texture_points(int(pos.shape[0]), ptr(pos) if pos.shape[0] else None, T, ptr(tri) if T else None,
                                                     int(texels), Q, ptr(face), ptr(point), ptr(footprint), ops._stream()))
    live = torch.nonzero(face.reshape(-1) >= 0).reshape(-1)
    return {"size": N, "squares_per_row": Q, "texels": int(texels), "face": face, "point": point, "footprint": footprint, "live": live,
            "uv": atlas_uv(T, texels, Q)}


def bake_textures(attributes: Callable[[Tensor, Tensor], Dict[str, Tensor]], atlas: Dict, chunk: int = DEFAULT_CHUNK) -> Dict[str, Tensor]:
    """`attributes`: (points [n,3], footprint [n]) -> {"diff" [n,3], "tint" [n,3], "roughness" [n], "pred_normals" [n,3]}, called on
    the live texels of `atlas` only, `chunk` at a time -> uint8 [N,N,3] images on the atlas' device: "diffuse", "tint", "roughness"
    (grey) and "normal" (object space, n * 0.5 + 0.5).  An unused texel holds 0.5 in the colour maps and roughness and (0, 0, 0) in
    the normal map: mid grey everywhere.  The bytes are rsn_visualize's (include/rsn.h): RSN_VIS_RGB, RSN_VIS_GRAY with lo 0 and hi
    1, RSN_VIS_UNIT, no alpha."""
    N = int(atlas["size"])
    live = atlas["live"]
    dev = atlas["point"].device
    pts, fp = atlas["point"].reshape(-1, 3), atlas["footprint"].reshape(-1)
    dense = {"diff": torch.full((N * N, 3), 0.5, device=dev), "tint": torch.full((N * N, 3), 0.5, device=dev),
             "roughness": torch.full((N * N,), 0.5, device=dev), "pred_normals": torch.zeros(N * N, 3, device=dev)}
    chunk = max(1, int(chunk))
    with torch.no_grad():
        for start in range(0, int(live.numel()), chunk):
            idx = live[start:start + chunk]
            got = attributes(pts[idx], fp[idx])
            for k, dst in dense.items():
                dst[idx] = got[k].to(torch.float32).reshape((idx.numel(),) + tuple(dst.shape[1:]))
    maps = {name: torch.empty(N, N, 3, device=dev, dtype=torch.uint8) for name in MAPS}
    with torch.cuda.device(dev):
        visualize(dense["diff"].reshape(N, N, 3), RSN_VIS_RGB, maps["diffuse"])
        visualize(dense["tint"].reshape(N, N, 3), RSN_VIS_RGB, maps["tint"])
        visualize(dense["roughness"].reshape(N, N), RSN_VIS_GRAY, maps["roughness"], lo=0.0, hi=1.0)
        visualize(dense["pred_normals"].reshape(N, N, 3), RSN_VIS_UNIT, maps["normal"])
    return maps


def footprint_bounds(spacing: Sequence[float], min_footprint: Optional[float] = None):
    """-> (lo, hi): the footprints a texel is queried with are clamped to [lo, hi]; hi = the largest grid spacing, lo = min_footprint,
    or hi / 8 when it is None -- a starting point that has not been measured on a scene.  ValueError unless 0 < lo <= hi."""
    hi = float(np.max(np.asarray(spacing, dtype=np.float32)))
    lo = hi / MIN_FOOTPRINT_FRACTION if min_footprint is None else float(min_footprint)
    if not (np.isfinite(lo) and 0.0 < lo <= hi):
        raise ValueError(f"min_footprint {lo!r}: need a value above 0 and at most the largest grid spacing {hi!r} (--min-footprint)")
    return lo, hi


def field_attributes(field, spacing: Sequence[float], min_footprint: Optional[float] = None,
                     chunk: int = DEFAULT_CHUNK) -> Callable[[Tensor, Tensor], Dict[str, Tensor]]:
    """The `attributes` of bake_textures for a field: every point is queried as an isotropic Gaussian of variance f^2 / 12 per axis
    with f = clamp(footprint, *footprint_bounds(spacing, min_footprint)), contracted like the model's samples and evaluated without a
    view direction, `chunk` points per launch.  min_footprint None: max(spacing) / 8, a starting point that has not been measured on
    a scene."""
    lo, hi = footprint_bounds(spacing, min_footprint)
    chunk = max(1, int(chunk))

    def attributes(points: Tensor, footprint: Tensor) -> Dict[str, Tensor]:
        n = int(points.shape[0])
        dev = points.device
        out = {"diff": torch.empty(n, 3, device=dev), "tint": torch.empty(n, 3, device=dev), "roughness": torch.empty(n, device=dev),
               "pred_normals": torch.empty(n, 3, device=dev)}
        with torch.no_grad():
            for start in range(0, n, chunk):
                p = points[start:start + chunk].to(torch.float32)
                f = footprint[start:start + chunk].to(torch.float32).clamp(lo, hi)
                cov = torch.diag_embed((f * f / 12.0)[:, None].expand(p.shape[0], 3))
                m, c = field.contract(p, cov)
                lv = field.evaluate_gaussians(m, torch.diagonal(c, dim1=-2, dim2=-1).contiguous(), None)
                for k, dst in out.items():
                    dst[start:start + p.shape[0]] = lv[k].reshape(dst[start:start + p.shape[0]].shape)
        return out

    return attributes


# ------------------------------------------------------------------------------------------------ OBJ
def _rows(fh, row_format: str, values: np.ndarray) -> None:
    """Write one text row per row of `values` [n, k]: the format of _ROWS_PER_FORMAT rows at a time is applied in one operation."""
    for start in range(0, values.shape[0], _ROWS_PER_FORMAT):
        part = values[start:start + _ROWS_PER_FORMAT]
        fh.write(((row_format * part.shape[0]) % tuple(part.reshape(-1).tolist())).encode("ascii"))


def obj_file_set(path: str) -> Dict[str, str]:
    """The six files of a textured export at `path` = DIR/NAME.obj: {"obj", "mtl", "diffuse", "tint", "roughness", "normal"}."""
    if not path.lower().endswith(".obj"):
        raise ValueError(f"{path!r}: a textured mesh is written as NAME.obj (with NAME.mtl and four NAME_<map>.png beside it)")
    stem = path[:-4]
    return {"obj": path, "mtl": stem + ".mtl", **{name: f"{stem}_{name}.png" for name in MAPS}}


def write_obj(path: str, mesh: Dict, atlas_uv: np.ndarray, maps: Dict) -> Dict[str, str]:
    """`mesh`: positions [V,3], triangles [T,3], pred_normals [V,3]; atlas_uv [T,3,2]; maps: the four uint8 [N,N,3] images of
    bake_textures (tensors or arrays) -> NAME.obj (mtllib, `v` and `vn` per vertex in %.9g, which round-trips fp32, three `vt` per
    face, `f v/vt/vn` 1-based), NAME.mtl (map_Kd: diffuse colour, map_Ks: tint, map_Pr: roughness, norm: the OBJECT-SPACE predicted
    normal as n * 0.5 + 0.5) and NAME_diffuse.png, NAME_tint.png, NAME_roughness.png, NAME_normal.png.  Every file goes through
    .tmp and os.replace; the same input gives the same bytes.  -> the paths (obj_file_set)."""
    from PIL import Image

    files = obj_file_set(path)
    name = os.path.basename(path)[:-4]
    pos, tri = _np(mesh["positions"], np.float32).reshape(-1, 3), _np(mesh["triangles"], np.int64).reshape(-1, 3)
    V, T = pos.shape[0], tri.shape[0]
    nrm = _np(mesh["pred_normals"], np.float32).reshape(V, 3)
    uv = np.ascontiguousarray(atlas_uv, dtype=np.float64).reshape(T * 3, 2)
    vt = 1 + np.arange(T * 3, dtype=np.int64).reshape(T, 3)
    corners = np.stack([tri + 1, vt, tri + 1], axis=-1).reshape(T, 9)  # v/vt/vn of the three corners
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)

    def obj(fh):
        fh.write(f"# reflect_sampling_nerf_amd export-mesh --texture\nmtllib {name}.mtl\n".encode("ascii"))
        _rows(fh, "v %.9g %.9g %.9g\n", pos.astype(np.float64))
        _rows(fh, "vn %.9g %.9g %.9g\n", nrm.astype(np.float64))
        _rows(fh, "vt %.12g %.12g\n", uv)
        fh.write(f"usemtl {name}\n".encode("ascii"))
        _rows(fh, "f %d/%d/%d %d/%d/%d %d/%d/%d\n", corners)

    def mtl(fh):
        lines = ["# reflect_sampling_nerf_amd export-mesh --texture",
                 "# map_Kd: the field's diffuse colour; map_Ks: its specular tint; map_Pr: its roughness (grey)",
                 "# norm: the field's predicted normal in OBJECT space (not tangent space), stored as n * 0.5 + 0.5",
                 f"newmtl {name}", "Ka 0 0 0", "Kd 1 1 1", "Ks 1 1 1", "illum 2"]
        lines += [f"{key} {name}_{m}.png" for key, m in MTL_KEYS]
        fh.write(("\n".join(lines) + "\n").encode("ascii"))

    def png(m):
        return lambda fh: Image.fromarray(_np(maps[m], np.uint8)).save(fh, format="PNG")

    for k, write in (("obj", obj), ("mtl", mtl), *((m, png(m)) for m in MAPS)):
        with replacing(files[k]) as tmp, open(tmp, "wb") as fh:
            write(fh)
    return files
