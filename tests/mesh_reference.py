"""Numpy restatement of the mesh-export contract of include/rsn.h (marching tetrahedra on the Kuhn split), in fp64
arithmetic on the fp32 input values, and the mesh properties the tests assert (closedness, Euler characteristic, signed
volume).  Written from the header's text, not from the kernel: the per-pattern triangle table is built from the six axis
permutations, and a triangle's orientation is decided GEOMETRICALLY (its normal against the direction from the
tetrahedron's inside vertices to its outside vertices), where the kernel uses permutation parities.

extract() emits in the header's order (vertices in ascending (v, dir); triangles by cell, permutation, in-tetrahedron
order); canonical() is the order-independent form two meshes are compared in."""
import itertools

import numpy as np

OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))  # dir 0..6 as (dx, dy, dz)
PERMUTATIONS = tuple(itertools.permutations(range(3)))  # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


def _corner(offset):  # local corner number: bit 0 = +x, bit 1 = +y, bit 2 = +z
    return offset[0] | (offset[1] << 1) | (offset[2] << 2)


DIR_OF_CORNER_DIFF = {_corner(o): d for d, o in enumerate(OFFSETS)}


def _tet_corners(perm):
    a, b, _ = perm
    return (0, 1 << a, (1 << a) | (1 << b), 7)


def _build_table():
    """pattern (bit L = corner L inside) -> list of triangles, each three edges (corner_lo, corner_hi), header order."""
    pos = np.array([[(L >> c) & 1 for c in range(3)] for L in range(8)], dtype=np.float64)
    table = []
    for pattern in range(256):
        tris = []
        for perm in PERMUTATIONS:
            tc = _tet_corners(perm)
            ins = [q for q in range(4) if (pattern >> tc[q]) & 1]
            outs = [q for q in range(4) if not (pattern >> tc[q]) & 1]
            if len(ins) in (0, 4):
                continue
            if len(ins) == 2:
                (a, b), (c, d) = ins, outs
                cand = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            else:
                lone = ins[0] if len(ins) == 1 else outs[0]
                j, k, l = [q for q in range(4) if q != lone]
                cand = [[(lone, j), (lone, k), (lone, l)]]
            outward = pos[[tc[q] for q in outs]].mean(0) - pos[[tc[q] for q in ins]].mean(0)
            for tri in cand:
                mid = [0.5 * (pos[tc[p]] + pos[tc[q]]) for p, q in tri]
                s = float(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), outward))
                assert abs(s) > 1e-9
                if s < 0:
                    tri = [tri[0], tri[2], tri[1]]
                tris.append([(tc[min(p, q)], tc[max(p, q)]) for p, q in tri])
        table.append(tris)
    return table


TABLE = _build_table()
TRI_COUNT = np.array([len(t) for t in TABLE], dtype=np.int64)
TRI_EDGES = np.zeros((256, 12, 3, 2), dtype=np.int64)
for _p, _t in enumerate(TABLE):
    if _t:
        TRI_EDGES[_p, : len(_t)] = np.array(_t, dtype=np.int64)
DIR_LUT = np.full(8, -1, dtype=np.int64)
for _k, _v in DIR_OF_CORNER_DIFF.items():
    DIR_LUT[_k] = _v


def extract(vol, iso, origin, spacing):
    """-> dict(positions float64 [V,3], vert_key int64 [V] = 8 v + dir, triangles int64 [T,3]).  vol: [nz, ny, nx]."""
    vol32 = np.asarray(vol, dtype=np.float32)
    nz, ny, nx = vol32.shape
    f = vol32.astype(np.float64)
    iso64 = float(np.float32(iso))
    o = np.asarray(origin, dtype=np.float32).astype(np.float64)
    s = np.asarray(spacing, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = vol32 >= np.float32(iso)  # NaN: False
    vidx = np.arange(nz * ny * nx, dtype=np.int64).reshape(nz, ny, nx)
    keys, pts = [], []
    for d, (dx, dy, dz) in enumerate(OFFSETS):
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cross = inside[lo] != inside[hi]
        v = vidx[lo][cross]
        f_lo, f_hi = f[lo][cross], f[hi][cross]
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            t = (iso64 - f_lo) / (f_hi - f_lo)
        t = np.where(np.isnan(t), 0.5, np.clip(t, 0.0, 1.0))
        ijk = np.stack([v % nx, (v // nx) % ny, v // (nx * ny)], axis=1).astype(np.float64)
        p_lo = o + s * ijk
        p_hi = o + s * (ijk + np.array([dx, dy, dz], dtype=np.float64))
        p = np.clip(p_lo + t[:, None] * (p_hi - p_lo), p_lo, p_hi)
        keys.append(v * 8 + d)
        pts.append(p)
    keys = np.concatenate(keys)
    pts = np.concatenate(pts, axis=0)
    order = np.argsort(keys, kind="stable")
    keys, pts = keys[order], pts[order]
    # cells, ascending lowest corner
    pattern = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.int64)
    for L in range(8):
        dx, dy, dz = L & 1, (L >> 1) & 1, (L >> 2) & 1
        pattern |= inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.int64) << L
    corner = vidx[:nz - 1, :ny - 1, :nx - 1].ravel()
    pattern = pattern.ravel()
    cnt = TRI_COUNT[pattern]
    cell = np.repeat(np.arange(pattern.size), cnt)
    within = np.arange(cell.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    e = TRI_EDGES[pattern[cell], within]  # [T, 3, 2] local corners
    llo, lhi = e[..., 0], e[..., 1]
    owner = corner[cell][:, None] + (llo & 1) + ((llo >> 1) & 1) * nx + ((llo >> 2) & 1) * nx * ny
    ekey = owner * 8 + DIR_LUT[llo ^ lhi]
    tri = np.searchsorted(keys, ekey)
    assert tri.size == 0 or np.array_equal(keys[tri], ekey), "a triangle names an edge that does not cross"
    return {"positions": pts.reshape(-1, 3), "vert_key": keys, "triangles": tri.reshape(-1, 3).astype(np.int64)}


def counts(vol, iso):
    """(number of surface vertices, number of triangles) of extract(), without building the mesh."""
    vol32 = np.asarray(vol, dtype=np.float32)
    nz, ny, nx = vol32.shape
    with np.errstate(invalid="ignore"):
        inside = vol32 >= np.float32(iso)
    n_vert = 0
    for dx, dy, dz in OFFSETS:
        n_vert += int(np.count_nonzero(inside[:nz - dz, :ny - dy, :nx - dx] != inside[dz:, dy:, dx:]))
    pattern = np.zeros((nz - 1, ny - 1, nx - 1), dtype=np.uint8)
    for L in range(8):
        dx, dy, dz = L & 1, (L >> 1) & 1, (L >> 2) & 1
        pattern |= inside[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx].astype(np.uint8) << np.uint8(L)
    return n_vert, int(TRI_COUNT[pattern].sum())


def canonical(triangles, vert_key):
    """Order-independent form: each triangle as its three vert_keys, rotated so that the smallest comes first (orientation
    kept), then the triangles sorted.  -> int64 [T,3]."""
    tri = np.asarray(vert_key, dtype=np.int64)[np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
    if tri.size == 0:
        return tri.reshape(0, 3)
    r = np.argmin(tri, axis=1)
    idx = (r[:, None] + np.arange(3)[None, :]) % 3
    tri = np.take_along_axis(tri, idx, axis=1)
    return tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))]


def _directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)


def unmatched_edges(triangles):
    """Directed edges (a, b) whose reverse (b, a) does not appear exactly once, or that appear more than once themselves.
    Empty for a closed, consistently oriented surface.  -> int64 [K,2]."""
    e = _directed_edges(triangles)
    if e.size == 0:
        return e
    base = int(e.max()) + 1
    code, rev = e[:, 0] * base + e[:, 1], e[:, 1] * base + e[:, 0]
    u, c = np.unique(code, return_counts=True)
    own = c[np.searchsorted(u, code)]
    pos = np.minimum(np.searchsorted(u, rev), len(u) - 1)
    back = np.where(u[pos] == rev, c[pos], 0)
    return e[(own != 1) | (back != 1)]


def euler_characteristic(triangles):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if t.size == 0:
        return 0
    e = np.sort(_directed_edges(t), axis=1)
    n_edges = len(np.unique(e[:, 0] * (int(t.max()) + 1) + e[:, 1]))
    return int(len(np.unique(t)) - n_edges + len(t))


def signed_volume(positions, triangles):
    """Volume enclosed by a closed mesh, positive when the normals point outwards (fp64)."""
    p = np.asarray(positions, dtype=np.float64)[np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


# ---- analytic volumes (fp32 [nz, ny, nx]) on the grid origin + spacing * (i, j, k); iso = 0, inside = positive
def grid_points(shape_xyz, origin, spacing):
    nx, ny, nz = shape_xyz
    o, s = np.asarray(origin, dtype=np.float32).astype(np.float64), np.asarray(spacing, dtype=np.float32).astype(np.float64)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return o[0] + s[0] * x, o[1] + s[1] * y, o[2] + s[2] * z


def sphere(shape_xyz, origin, spacing, centre, radius):
    x, y, z = grid_points(shape_xyz, origin, spacing)
    return (radius - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def torus(shape_xyz, origin, spacing, centre, major, minor):
    x, y, z = grid_points(shape_xyz, origin, spacing)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - major
    return (minor - np.sqrt(q ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def gyroid(shape_xyz, origin, spacing):
    x, y, z = grid_points(shape_xyz, origin, spacing)
    return (np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x)).astype(np.float32)


# ---- a reader for exactly the PLY files mesh.write_ply promises
def parse_ply(path):
    """A reader for exactly what write_ply promises: -> (vertex dict of arrays, faces [T,3], header lines)."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").strip().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    elements, props = [], {}
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            elements.append((w[1], int(w[2])))
            props[w[1]] = []
        elif w[0] == "property":
            props[elements[-1][0]].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    kinds = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(name, kinds[kind]) for kind, name in props["vertex"]])
    nv, nf = elements[0][1], elements[1][1]
    vert = np.frombuffer(blob, dtype=vdt, count=nv, offset=end)
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    face = np.frombuffer(blob, dtype=fdt, count=nf, offset=end + nv * vdt.itemsize)
    assert end + nv * vdt.itemsize + nf * fdt.itemsize == len(blob)
    assert np.all(face["n"] == 3)
    return {n: vert[n] for n in vdt.names}, face["v"], lines
