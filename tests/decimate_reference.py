"""Numpy restatement of the decimation contract of include/rsn.h (vertex clustering): the fp32 steps with np.float32, the integer
sums with int64, the representative in fp64 -- and of decimate.search_cells.  Written from the header's text, not from the kernels:
groups are formed by a lexicographic sort of the three CELL IDS (the library sorts a key of compact ranks), the orientation is the
parity of the sorting permutation (the library counts ascents around the cycle), and the sums are np.add.at.

decimate() returns what the device must return by bits and order."""
import numpy as np

ONE = np.float32(2.0 ** 20)
MAX_OCCUPIED = 1 << 21


def axis_cells(p, o, c, n):
    """One axis: positions p (fp32 array), origin o, cell size c, n cells -> (cell index int64, fixed-point offset q int64)."""
    p, o, c = np.asarray(p, dtype=np.float32), np.float32(o), np.float32(c)
    with np.errstate(all="ignore"):
        u = ((p - o).astype(np.float32) / c).astype(np.float32)
        u = np.where(np.isfinite(u), u, np.float32(0.0)).astype(np.float32)
        i = np.clip(np.floor(u).astype(np.float64), 0.0, float(n - 1)).astype(np.int64)
        f = (u - i.astype(np.int32).astype(np.float32)).astype(np.float32)
        q = np.clip(np.rint((f * ONE).astype(np.float32)).astype(np.float64), 0.0, float(ONE)).astype(np.int64)
    return i, q


def vertex_cells(positions, origin, cell, dims):
    """-> (flat cell id int64 [V], index int64 [V,3], q int64 [V,3])."""
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    idx, q = np.zeros(pos.shape, dtype=np.int64), np.zeros(pos.shape, dtype=np.int64)
    for a in range(3):
        idx[:, a], q[:, a] = axis_cells(pos[:, a], origin[a], cell[a], dims[a])
    cx, cy, _ = (int(d) for d in dims)
    return (idx[:, 2] * cy + idx[:, 1]) * cx + idx[:, 0], idx, q


def representatives(cells, origin, cell, dims, flat, q):
    """The representative of each of the ascending, occupied `cells` -> fp32 [len(cells), 3]."""
    cx, cy, _ = (int(d) for d in dims)
    slot = np.searchsorted(cells, flat)
    mine = (slot < len(cells)) & (cells[np.minimum(slot, len(cells) - 1)] == flat) if len(cells) else np.zeros(len(flat), dtype=bool)
    S = np.zeros((len(cells), 3), dtype=np.int64)
    m = np.zeros(len(cells), dtype=np.int64)
    np.add.at(S, slot[mine], q[mine])
    np.add.at(m, slot[mine], 1)
    ijk = np.stack([cells % cx, (cells // cx) % cy, cells // (cx * cy)], axis=1).astype(np.float64)
    o = np.asarray(origin, dtype=np.float32).astype(np.float64)
    c = np.asarray(cell, dtype=np.float32).astype(np.float64)
    mean = (S.astype(np.float64) / m.astype(np.float64)[:, None]) * 2.0 ** -20
    return (o + c * (ijk + mean)).astype(np.float32)


def resolve(triangles, flat, n_vertices):
    """The triangle rule -> (survivor mask [T], degenerate count, cancelled pairs)."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    T = len(tri)
    valid = np.all((tri >= 0) & (tri < n_vertices), axis=1)
    c = np.where(valid[:, None], flat[np.clip(tri, 0, max(n_vertices - 1, 0))] if n_vertices else 0, -1)
    live = valid & (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    keep = np.zeros(T, dtype=bool)
    t = np.flatnonzero(live)
    if len(t) == 0:
        return keep, T, 0
    c = c[t]
    perm = np.argsort(c, axis=1, kind="stable")
    s = np.take_along_axis(c, perm, axis=1)
    # parity of the sorting permutation of three distinct values: even <=> it is a rotation <=> perm[1] == (perm[0] + 1) % 3
    plus = perm[:, 1] == (perm[:, 0] + 1) % 3
    order = np.lexsort((t, s[:, 2], s[:, 1], s[:, 0]))  # groups together, ascending original index inside
    s, plus, t = s[order], plus[order], t[order]
    head = np.ones(len(t), dtype=bool)
    head[1:] = np.any(s[1:] != s[:-1], axis=1)
    gid = np.cumsum(head) - 1
    n_plus = np.bincount(gid, weights=plus).astype(np.int64)
    n_minus = np.bincount(gid, weights=~plus).astype(np.int64)
    net = n_plus - n_minus
    # the position of every triangle among those of its own orientation in its group
    start = np.flatnonzero(head)[gid]
    cum_plus = np.cumsum(plus) - plus
    nth_plus = cum_plus - cum_plus[start]
    cum_minus = np.cumsum(~plus) - (~plus)
    nth_minus = cum_minus - cum_minus[start]
    nth = np.where(plus, nth_plus, nth_minus)
    majority = np.where(net[gid] > 0, plus, ~plus) & (net[gid] != 0)
    keep[t[majority & (nth < np.abs(net[gid]))]] = True
    return keep, int(T - len(t)), int(np.minimum(n_plus, n_minus).sum())


def decimate(positions, triangles, origin, cell, dims):
    """-> dict(positions fp32 [V',3], triangles int32 [T',3], counts = (vertices, triangles, degenerate, cancelled pairs), cells int64
    [V'] the cell id of every output vertex, occupied = the number of occupied cells)."""
    pos = np.asarray(positions, dtype=np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = len(pos)
    if V == 0 or len(tri) == 0:
        return {"positions": np.zeros((0, 3), np.float32), "triangles": np.zeros((0, 3), np.int32), "counts": (0, 0, 0, 0),
                "cells": np.zeros(0, np.int64), "occupied": 0}
    flat, _, q = vertex_cells(pos, origin, cell, dims)
    keep, degenerate, cancelled = resolve(tri, flat, V)
    kept = tri[keep]
    cells = np.unique(flat[kept.reshape(-1)])
    out_tri = np.searchsorted(cells, flat[kept]).astype(np.int32).reshape(-1, 3)
    out_pos = representatives(cells, origin, cell, dims, flat, q)
    return {"positions": out_pos, "triangles": out_tri, "counts": (len(cells), len(kept), degenerate, cancelled), "cells": cells,
            "occupied": len(np.unique(flat))}


def cell_frame(bounds, n):
    """pointcloud.cell_frame, restated: n cells, n intervals -> ((nx, ny, nz), origin fp32 [3], cell fp32 [3])."""
    dims = (int(n),) * 3 if np.ndim(n) == 0 else tuple(int(x) for x in n)
    b = np.asarray(bounds, dtype=np.float64).reshape(6)
    return dims, b[:3].astype(np.float32), ((b[3:] - b[:3]) / np.asarray(dims, dtype=np.float64)).astype(np.float32)


def survivors(positions, triangles, bounds, n):
    dims, origin, cell = cell_frame(bounds, n)
    d = decimate(positions, triangles, origin, cell, dims)
    return d["counts"][1] if d["occupied"] <= MAX_OCCUPIED else None


def search_cells(count, target_faces, max_cells):
    """decimate.search_cells, restated -> (n, probes [(n, count)], over)."""
    probes, seen = [], {}

    def fits(n):
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
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        n = lo
    while not fits(n) and n > 2:
        n -= 1
    return n, probes, not fits(n)


def decimate_to(positions, triangles, bounds, target_faces, max_cells):
    n, probes, over = search_cells(lambda k: survivors(positions, triangles, bounds, k), target_faces, max_cells)
    dims, origin, cell = cell_frame(bounds, n)
    return decimate(positions, triangles, origin, cell, dims), {"n": n, "probes": probes, "over_budget": over}


def edge_imbalance(triangles):
    """Directed edges (a, b) that do not occur exactly as often as (b, a) -> their number (0 for a balanced mesh)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if t.size == 0:
        return 0
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)
    base = int(e.max()) + 1
    fwd, fc = np.unique(e[:, 0] * base + e[:, 1], return_counts=True)
    rev = (fwd % base) * base + fwd // base
    at = np.minimum(np.searchsorted(fwd, rev), len(fwd) - 1)
    back = np.where(fwd[at] == rev, fc[at], 0)
    return int(np.count_nonzero(fc != back))


# ---- the inputs both test files share: the suite's analytic volumes (tests/test_mesh_cpu.py, test_mesh_gpu.py) through the
# reference extractor, positions as fp32
BOX = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
GYROID_ORIGIN, GYROID_SPACING, GYROID_SHAPE = (-3.1, -2.7, -1.9), (0.37, 0.41, 0.29), (19, 23, 17)
GYROID_BOX = tuple(GYROID_ORIGIN) + tuple(o + s * (n - 1) for o, s, n in zip(GYROID_ORIGIN, GYROID_SPACING, GYROID_SHAPE))
_meshes = {}


def box_grid(n):
    """n vertices per axis over BOX -> (shape, origin, spacing) as the extractor takes them."""
    h = np.float32(2.0 / (n - 1))
    return (n, n, n), (-1.0, -1.0, -1.0), (h, h, h)


def sphere_volume(n):
    from tests import mesh_reference as mref

    return mref.sphere(*box_grid(n), (0.03, -0.02, 0.05), 0.8)


def fixture_mesh(name):
    """"sphere_24", "sphere_33", "torus_33" (closed, in BOX) or "gyroid" (ragged 19 x 23 x 17 grid, open, in GYROID_BOX)
    -> (positions fp32 [V,3], triangles int64 [T,3]), extracted once."""
    from tests import mesh_reference as mref

    if name not in _meshes:
        if name == "gyroid":
            m = mref.extract(mref.gyroid(GYROID_SHAPE, GYROID_ORIGIN, GYROID_SPACING), 0.05, GYROID_ORIGIN, GYROID_SPACING)
            assert len(mref.unmatched_edges(m["triangles"])) > 0  # open
        else:
            kind, n = name.split("_")
            shape, origin, spacing = box_grid(int(n))
            vol = sphere_volume(int(n)) if kind == "sphere" else mref.torus(shape, origin, spacing, (0.02, 0.01, -0.03), 0.55, 0.22)
            m = mref.extract(vol, 0.0, origin, spacing)
            assert len(mref.unmatched_edges(m["triangles"])) == 0  # closed
        _meshes[name] = (m["positions"].astype(np.float32), m["triangles"])
    return _meshes[name]
