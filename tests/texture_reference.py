"""numpy restatement of the texture atlas of include/rsn.h ("texture atlas"): the layout, the point and footprint arithmetic in fp32,
one rounding per step in the header's order; a bilinear sampler; a minimal OBJ / MTL parser.  No torch, no device."""
import os

import numpy as np

F = np.float32


def squares_per_row(n_triangles):
    """Q = max(1, ceil(sqrt(ceil(T / 2)))) in integers."""
    S = (int(n_triangles) + 1) // 2
    Q = 1
    while Q * Q < S:
        Q += 1
    return Q


def classify(P, a, b):
    """Integer arrays a (column), b (row) inside a square -> (upper, live)."""
    upper = a + b >= P - 1
    live = np.where(upper, (a >= 2) & (b >= 2), (a <= P - 3) & (b <= P - 3))
    return upper, live


def corners(P):
    """Texel centres (column, row) of the corners 0, 1, 2 of the lower and of the upper triangle of a square -> int [2,3,2]."""
    return np.array([[[0, 0], [P - 3, 0], [0, P - 3]], [[P - 1, P - 1], [2, P - 1], [P - 1, 2]]], dtype=np.int64)


def texel_uv(P, a, b, upper):
    """(u, v) of texels as fp32: one int-to-float conversion (exact) and one division each."""
    d = F(P - 3)
    u = np.where(upper, P - 1 - a, a).astype(F) / d
    v = np.where(upper, P - 1 - b, b).astype(F) / d
    return u.astype(F), v.astype(F)


def texture_points(positions, triangles, P, Q=None):
    """-> {"size", "squares_per_row", "face" int32 [N,N], "point" fp32 [N,N,3], "footprint" fp32 [N,N]} as rsn_texture_points
    writes them."""
    pos = np.ascontiguousarray(positions, dtype=F).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = len(pos), len(tri)
    Q = squares_per_row(T) if Q is None else int(Q)
    N = Q * P
    row, col = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    sx, a, sy, b = col // P, col % P, row // P, row % P
    upper, live = classify(P, a, b)
    t = 2 * (sy * Q + sx) + upper
    used = live & (t < T)
    tt = np.where(used, t, 0)
    idx = tri[tt] if T else np.zeros((N, N, 3), dtype=np.int64)
    used &= np.all((idx >= 0) & (idx < V), axis=-1)
    idx = np.where(used[..., None], idx, 0)
    p0, p1, p2 = (pos[idx[..., k]] if V else np.zeros((N, N, 3), dtype=F) for k in range(3))
    u, v = texel_uv(P, a, b, upper)
    with np.errstate(all="ignore"):
        w0 = ((F(1.0) - u).astype(F) - v).astype(F)
        point = (((w0[..., None] * p0).astype(F) + (u[..., None] * p1).astype(F)).astype(F) + (v[..., None] * p2).astype(F)).astype(F)

        def length(p, q):
            d = (p - q).astype(F)
            sq = (d * d).astype(F)
            return np.sqrt(((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)).astype(F)

        h = (np.maximum(length(p1, p0), length(p2, p0)) / F(P - 3)).astype(F)
    face = np.where(used, t, -1).astype(np.int32)
    return {"size": N, "squares_per_row": Q, "face": face, "point": np.where(used[..., None], point, F(0.0)).astype(F),
            "footprint": np.where(used, h, F(0.0)).astype(F)}


def corner_uv(T, P, Q):
    """OBJ coordinates of the corners -> float64 [T,3,2]: vt = ((col + 0.5) / N, 1 - (row + 0.5) / N)."""
    N = Q * P
    t = np.arange(T)
    q = t // 2
    c = corners(P)[t % 2]  # [T,3,2]
    col, row = (q % Q)[:, None] * P + c[..., 0], (q // Q)[:, None] * P + c[..., 1]
    return np.stack([(col + 0.5) / N, 1.0 - (row + 0.5) / N], axis=-1)


def quantise(x):
    """rsn_visualize's q(sat(x)) in fp32: sat, then (uint8)(int)(v * 255 + 0.5), a multiply and an add."""
    x = np.asarray(x, dtype=F)
    s = np.where(np.isnan(x) | (x <= 0), F(0.0), np.where(x > 1, F(1.0), x)).astype(F)
    return ((s * F(255.0)).astype(F) + F(0.5)).astype(F).astype(np.int32).astype(np.uint8)


def taps_at(x, y, N):
    """The four taps of bilinear filtering at texel coordinates (x, y) [n] (texel centres at the integers, x along a row, clamped at
    the border) of an N x N image -> rows int [n,4], cols int [n,4], weights float64 [n,4]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    cols = np.clip(np.stack([x0, x0 + 1, x0, x0 + 1], axis=1), 0, N - 1)
    rows = np.clip(np.stack([y0, y0, y0 + 1, y0 + 1], axis=1), 0, N - 1)
    w = np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], axis=1)
    return rows, cols, w


def bilinear_taps(uv, N):
    """taps_at for OBJ coordinates uv [n,2]: image row 0 at the top, texel centres at (i + 0.5) / N."""
    uv = np.asarray(uv, dtype=np.float64)
    return taps_at(uv[:, 0] * N - 0.5, (1.0 - uv[:, 1]) * N - 0.5, N)


def bilinear(image, uv):
    """image [N,N] or [N,N,C] (any real dtype) sampled at uv [n,2] -> float64 [n] or [n,C]."""
    img = np.asarray(image, dtype=np.float64)
    rows, cols, w = bilinear_taps(uv, img.shape[0])
    taps = img[rows, cols]
    return (taps * (w if taps.ndim == 2 else w[..., None])).sum(axis=1)


def parse_obj(path):
    """-> {"mtllib", "usemtl", "v" [V,3] fp32 (parsed as float, cast), "vn" [Vn,3], "vt" [Vt,2] float64, "fv", "fvt", "fvn" int [T,3],
    0-based}."""
    out = {"mtllib": None, "usemtl": None}
    rows = {"v": [], "vn": [], "vt": [], "f": []}
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] in ("mtllib", "usemtl"):
                out[w[0]] = w[1]
            elif w[0] == "f":
                rows["f"].append([[int(x) for x in c.split("/")] for c in w[1:]])
            elif w[0] in rows:
                rows[w[0]].append([float(x) for x in w[1:]])
            else:
                raise ValueError(f"{path}: unknown statement {w[0]!r}")
    out["v"] = np.array(rows["v"], dtype=np.float64).reshape(-1, 3).astype(F)
    out["vn"] = np.array(rows["vn"], dtype=np.float64).reshape(-1, 3).astype(F)
    out["vt"] = np.array(rows["vt"], dtype=np.float64).reshape(-1, 2)
    f = np.array(rows["f"], dtype=np.int64).reshape(-1, 3, 3) - 1
    out["fv"], out["fvt"], out["fvn"] = f[..., 0], f[..., 1], f[..., 2]
    return out


def parse_mtl(path):
    """-> {"newmtl": name, key: value string for every other statement}, comments in "comments"."""
    out = {"comments": []}
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith("#"):
                out["comments"].append(line)
            elif line:
                k, _, v = line.partition(" ")
                out[k] = v
    return out


def file_set(path):
    stem = path[:-4]
    return [path, stem + ".mtl"] + [f"{stem}_{m}.png" for m in ("diffuse", "tint", "roughness", "normal")]


def read_all(paths):
    return [open(p, "rb").read() if os.path.exists(p) else None for p in paths]


# ---------------------------------------------------------------------------------------------- the round trip of the tests
def triangle_soup(rng, T, scale=1.0):
    """T random triangles with three vertices of their own each -> positions fp32 [3T,3], triangles int32 [T,3]."""
    return (rng.normal(size=(3 * T, 3)) * scale).astype(F), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def linear_function(positions, rng):
    """f(p) = c . p + d with a random direction c, scaled so that its values at `positions` span exactly [1/3, 2/3] -> (c [3], d),
    float64.  On a triangle a linear function lies between its corner values; at a live texel w0 >= -1 and u, v in [0, 1], so the
    extrapolation stays inside [1/3 + 1/3 - 2/3, 2/3 + 2/3 - 1/3] = [0, 1]."""
    c = rng.normal(size=3)
    g = np.asarray(positions, dtype=np.float64) @ c
    k = (1.0 / 3.0) / (g.max() - g.min())
    return c * k, 1.0 / 3.0 - g.min() * k


def interior_barycentrics(rng, n):
    """n random points inside a triangle as barycentric weights (w0, w1, w2) -> float64 [n,3]."""
    uv = rng.uniform(size=(n, 2))
    uv = np.where((uv.sum(axis=1) > 1.0)[:, None], 1.0 - uv, uv)
    return np.concatenate([1.0 - uv.sum(axis=1, keepdims=True), uv], axis=1)


def round_trip_error(image, face, uv, positions, triangles, c, d, bary):
    """Sample `image` [N,N] (values in [0, 1]) bilinearly at the points `bary` of every triangle, through the corner coordinates
    uv [T,3,2], and compare with f(p) = c . p + d at the same points of the mesh -> the largest |difference|.  Asserts property (a)
    on the way: every tap with a weight above 1e-9 (the uv arithmetic is float64) is a texel whose face is the triangle."""
    pos = np.asarray(positions, dtype=np.float64)
    worst = 0.0
    for t, tri in enumerate(np.asarray(triangles)):
        at = bary @ uv[t]
        rows, cols, w = bilinear_taps(at, image.shape[0])
        assert np.all((face[rows, cols] == t) | (w <= 1e-9)), f"triangle {t}: a tap outside its live texels"
        worst = max(worst, float(np.abs(bilinear(image, at) - ((bary @ pos[tri]) @ c + d)).max()))
    return worst
