"""Reduce an extracted mesh to a face budget by vertex clustering, on the device (rsn_decimate_* of include/rsn.h).

    python -m reflect_sampling_nerf_amd.trainer export-mesh ... [--decimate-cells N | --target-faces N]

A regular grid of cluster cells (pointcloud.cell_frame: n cells, n intervals over the bounds) covers the box.  All vertices in a cell
merge into one, at the mean of the cell's vertices; triangles that collapse disappear; triangles that end up on the same three cells
cancel in opposite pairs and otherwise keep their multiplicity (the rule, and why it is not "drop duplicates": include/rsn.h and
DESIGN.md 4.22).  A closed input gives an output whose directed edges balance; manifoldness and the genus are not promised.

The field is the source of every attribute, so a reduced mesh needs no attribute interpolation: export_mesh queries the field at the
new vertices, with the CLUSTER CELL as the footprint -- a merged vertex stands for a cell.  That footprint is a design rule; it has
not been measured against a scene, and neither has any effect of the reduction on rendered appearance, nor the quality of the meshes
against an edge-collapse simplifier (what pymeshlab does behind ns-export's --target-num-faces).

Deterministic: the same bytes in the same order from run to run.  The one step outside the library is a stable sort of one int64
key per triangle (torch.sort on the device).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _abi, ops
from ._abi import check, float3, ptr

MAX_OCCUPIED = 1 << 21  # occupied cells whose ranks fit the sort key (include/rsn.h)
COUNT_NAMES = ("vertices", "triangles", "degenerate", "cancelled_pairs", "occupied_cells")


class _Run:
    """One pass of the library calls over one mesh and one grid of cells: the buffers they share."""

    def __init__(self, mesh: Dict[str, Tensor], bounds: Sequence[float], cells: Union[int, Sequence[int]]):
        from .pointcloud import cell_frame

        pos, tri = mesh["positions"], mesh["triangles"]
        if pos.dtype != torch.float32 or pos.device.type != "cuda" or pos.dim() != 2 or pos.shape[1] != 3:
            raise _abi.RsnError("decimate: positions must be an fp32 [V,3] tensor on a cuda (ROCm) device")
        if tri.dtype != torch.int32 or tri.device != pos.device or tri.dim() != 2 or tri.shape[1] != 3:
            raise _abi.RsnError("decimate: triangles must be an int32 [T,3] tensor on the device of positions")
        self.pos, self.tri = pos.contiguous(), tri.contiguous()
        self.dims, self.origin, self.cell = cell_frame(bounds, cells)
        self.V, self.T = int(pos.shape[0]), int(tri.shape[0])
        self.lib = _abi.load_library()
        self.nbytes = int(self.lib.rsn_decimate_workspace_bytes(self.V, self.T, *self.dims))
        if self.nbytes == 0:
            check(-1)
        dev = pos.device
        self.ws = torch.empty((self.nbytes + 7) // 8, device=dev, dtype=torch.int64)  # 8-byte aligned
        self.counts = torch.empty(5, device=dev, dtype=torch.int32)
        self.keys = torch.empty(self.T, device=dev, dtype=torch.int64)

    def _frame(self):
        return float3(self.origin), float3(self.cell), *self.dims, ptr(self.ws), self.nbytes

    def resolve(self, mark: Optional[Callable[[str], None]] = None) -> None:
        """The cluster and triangle stages: afterwards counts holds the survivors, the degenerate triangles, the cancelled pairs and
        the occupied cells."""
        lib, st = self.lib, ops._stream()
        check(lib.rsn_decimate_cluster(self.V, ptr(self.pos), self.T, ptr(self.tri), *self._frame(), ptr(self.keys), ptr(self.counts), st))
        if mark:
            mark("cluster")
        sorted_keys, order = torch.sort(self.keys, stable=True)  # the one step outside the library
        if mark:
            mark("sort")
        check(lib.rsn_decimate_resolve(self.V, self.T, *self.dims, ptr(sorted_keys), ptr(order), ptr(self.ws), self.nbytes,
                                       ptr(self.counts), st))
        if mark:
            mark("resolve")

    def read_counts(self) -> Dict[str, int]:
        """The one device-to-host read."""
        c = dict(zip(COUNT_NAMES, (int(x) for x in self.counts.tolist())))
        c["supported"] = c["occupied_cells"] <= MAX_OCCUPIED
        return c

    def finish(self, mark: Optional[Callable[[str], None]] = None) -> Tuple[Dict[str, Tensor], Dict[str, int]]:
        lib, st = self.lib, ops._stream()
        check(lib.rsn_decimate_count(self.V, self.T, ptr(self.tri), *self.dims, ptr(self.ws), self.nbytes, ptr(self.counts), st))
        if mark:
            mark("count")
        c = self.read_counts()
        if not c["supported"]:
            raise _abi.RsnError(f"librsn_hip error {-2}: decimate: {c['occupied_cells']} occupied cells of {' x '.join(map(str, self.dims))}: "
                                f"more than 2^21 (the ranks of three cells share one 64-bit sort key); use fewer cells")
        dev = self.pos.device
        out_pos = torch.empty(c["vertices"], 3, device=dev, dtype=torch.float32)
        out_tri = torch.empty(c["triangles"], 3, device=dev, dtype=torch.int32)
        check(lib.rsn_decimate_emit(self.V, ptr(self.pos), self.T, ptr(self.tri), *self._frame(), c["vertices"], c["triangles"],
                                    ptr(out_pos) if c["vertices"] else None, ptr(out_tri) if c["triangles"] else None, st))
        if mark:
            mark("emit")
        return {"positions": out_pos, "triangles": out_tri}, c


def _stats(run: _Run, c: Dict[str, int]) -> dict:
    return {"cells": [int(n) for n in run.dims], "cell_size": [float(x) for x in run.cell], "vertices_in": run.V, "triangles_in": run.T,
            **{k: c[k] for k in COUNT_NAMES}}


def decimate(mesh: Dict[str, Tensor], bounds: Sequence[float], cells: Union[int, Sequence[int]],
             mark: Optional[Callable[[str], None]] = None) -> Dict:
    """`mesh`: {"positions" fp32 [V,3], "triangles" int32 [T,3], ...} on the device; cells: an int or (cx, cy, cz), the cluster cells
    per axis of pointcloud.cell_frame(bounds, cells) -> {"positions", "triangles", "stats"}: the clustered mesh (vert_key and every
    other per-vertex entry lose their meaning and are dropped) and stats = {cells, cell_size, vertices_in, triangles_in, vertices,
    triangles, degenerate, cancelled_pairs, occupied_cells}.  One device-to-host read: the counts, to size the outputs.
    mark: called with a stage's name (cluster, sort, resolve, count, emit) after its launches are enqueued."""
    run = _Run(mesh, bounds, cells)
    run.resolve(mark)
    out, c = run.finish(mark)
    out["stats"] = _stats(run, c)
    return out


def survivors(mesh: Dict[str, Tensor], bounds: Sequence[float], cells: Union[int, Sequence[int]]) -> Optional[int]:
    """The number of triangles decimate would leave, from the cluster and triangle stages alone and one read -> None when the grid
    has more occupied cells than the library takes."""
    run = _Run(mesh, bounds, cells)
    run.resolve()
    c = run.read_counts()
    return c["triangles"] if c["supported"] else None


def search_cells(count: Callable[[int], Optional[int]], target_faces: int, max_cells: int) -> Tuple[int, List[Tuple[int, Optional[int]]], bool]:
    """The cells per axis for a face budget: the n in [2, max_cells] that a bisection finds for "the largest n whose count is at most
    target_faces", taking the count as growing with n.  count(n) -> the survivors at n cells per axis, or None where n cannot be run,
    which counts as above every budget.  -> (n, [(n probed, its count), ...] in the order probed, over): `over` says that even n = 2
    exceeds the budget (n is 2 then).

    max_cells is probed first and taken if it fits; else 2 (over, if it does not fit); else the bisection keeps a lower end that fits
    and an upper end that does not, so the n it ends on fits and n + 1 does not.  The count is not strictly monotone in n, so a
    larger n that fits may exist; none is looked for.  The walk that follows -- while the count exceeds the budget and n > 2, take
    n - 1 -- is a guard: the lower end is always a probed n, so no input reaches it."""
    target_faces, max_cells = int(target_faces), int(max_cells)
    if target_faces < 1 or max_cells < 2:
        raise ValueError(f"target_faces {target_faces} / max_cells {max_cells}: need a budget of at least 1 and at least 2 cells per axis")
    probes: List[Tuple[int, Optional[int]]] = []
    seen: Dict[int, Optional[int]] = {}

    def fits(n: int) -> bool:
        if n not in seen:
            seen[n] = count(n)
            probes.append((n, seen[n]))
        return seen[n] is not None and seen[n] <= target_faces

    if fits(max_cells):
        n = max_cells
    elif not fits(2):
        n = 2
    else:
        lo, hi = 2, max_cells
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fits(mid):
                lo = mid
            else:
                hi = mid
        n = lo
    while not fits(n) and n > 2:
        n -= 1
    return n, probes, not fits(n)


def decimate_to(mesh: Dict[str, Tensor], bounds: Sequence[float], target_faces: int, max_cells: int,
                mark: Optional[Callable[[str], None]] = None) -> Tuple[Dict[str, Tensor], dict]:
    """Cluster with the same n cells on every axis, n chosen by search_cells for at most target_faces triangles -> (mesh, stats):
    the mesh of decimate at that n (without its stats entry) and stats = decimate's, with n, target_faces, max_cells, probes
    ([[n, count], ...]: each one run of the cluster and triangle stages and one read), the count reached (triangles) and
    over_budget (true when even two cells per axis leave more than the budget: the result is that mesh)."""
    n, probes, over = search_cells(lambda k: survivors(mesh, bounds, k), target_faces, max_cells)
    if mark:
        mark("search")
    out = decimate(mesh, bounds, n, mark)
    stats = out.pop("stats")
    stats.update(n=n, target_faces=int(target_faces), max_cells=int(max_cells), probes=[[k, c] for k, c in probes], over_budget=over)
    return out, stats
