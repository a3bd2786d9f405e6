"""Numpy restatement of the TSDF-fusion contract of include/rsn.h (rsn_tsdf_integrate) -- fp32, every step one numpy fp32
operation in the header's order, so that the device result can be compared bit for bit -- and of mesh.tsdf_volume /
mesh.drop_unobserved.  Written from the header's text, not from the kernel.  Also the test scenes: look-at cameras in the ray
convention of the header and analytic median-depth maps of a sphere."""
import numpy as np

from tests.mesh_reference import OFFSETS

F32 = np.float32


def integrate(tsdf, weight, origin, spacing, c2w, height, width, fx, fy, cx, cy, depth, trunc, near):
    """tsdf / weight: fp32 [nz, ny, nx]; c2w [n,3,4]; depth [n, H*W] -> new (tsdf, weight); the inputs are not modified."""
    T = np.array(tsdf, dtype=F32, copy=True)
    Wt = np.array(weight, dtype=F32, copy=True)
    nz, ny, nx = T.shape
    o, s = np.asarray(origin, dtype=F32), np.asarray(spacing, dtype=F32)
    c2w = np.asarray(c2w, dtype=F32).reshape(-1, 3, 4)
    depth = np.asarray(depth, dtype=F32).reshape(len(c2w), int(height) * int(width))
    fx, fy, cx, cy, trunc, near = (F32(x) for x in (fx, fy, cx, cy, trunc, near))
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = [o[a] + s[a] * idx.astype(F32) for a, idx in enumerate((i, j, k))]
    assert all(x.dtype == F32 for x in p)
    with np.errstate(all="ignore"):
        for n, m in enumerate(c2w):
            q = [p[a] - m[a, 3] for a in range(3)]
            cam = [(m[0, c] * q[0] + m[1, c] * q[1]) + m[2, c] * q[2] for c in range(3)]
            z = -cam[2]
            ok = z > 0
            u = (fx * cam[0]) / z + cx
            v = cy - (fy * cam[1]) / z
            ok &= (u >= 0) & (u < F32(width)) & (v >= 0) & (v < F32(height))
            r = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
            ok &= ~(r < near)
            x = np.where(ok, np.floor(u), 0).astype(np.int64)
            y = np.where(ok, np.floor(v), 0).astype(np.int64)
            D = depth[n][y * int(width) + x]
            ok &= np.isfinite(D)
            sd = D - r
            ok &= ~(sd < -trunc)
            d = np.minimum(F32(1.0), sd / trunc)
            Wn = Wt + F32(1.0)
            Tn = (T * Wt + d) / Wn
            assert Tn.dtype == F32 and Wn.dtype == F32 and u.dtype == F32 and r.dtype == F32
            T = np.where(ok, Tn, T)
            Wt = np.where(ok, Wn, Wt)
    return T, Wt


def tsdf_volume(tsdf, weight, min_weight=1.0):
    return np.where(np.asarray(weight) >= min_weight, -np.asarray(tsdf, dtype=F32), F32(-1.0)).astype(F32)


def drop_unobserved(mesh, weight, dims, min_weight=1.0):
    """mesh: positions [V,3], vert_key [V], triangles [T,3] -> the same keys, filtered: a vertex is valid iff both ends of its
    grid edge have weight >= min_weight; triangles with three valid vertices stay; unreferenced vertices go; stable renumbering.
    Loops over entries on purpose: the package's form is vectorised."""
    nx, ny, nz = (int(d) for d in dims)
    w = np.asarray(weight).reshape(nz, ny, nx)
    valid = []
    for key in np.asarray(mesh["vert_key"], dtype=np.int64):
        v, d = divmod(int(key), 8)
        i, j, k = v % nx, (v // nx) % ny, v // (nx * ny)
        dx, dy, dz = OFFSETS[d]
        valid.append(bool(w[k, j, i] >= min_weight and w[k + dz, j + dy, i + dx] >= min_weight))
    tris = [t for t in np.asarray(mesh["triangles"], dtype=np.int64).reshape(-1, 3) if all(valid[a] for a in t)]
    used = sorted({int(a) for t in tris for a in t})
    new_id = {old: new for new, old in enumerate(used)}
    tri = np.array([[new_id[int(a)] for a in t] for t in tris], dtype=np.int64).reshape(-1, 3)
    return {"positions": np.asarray(mesh["positions"])[used].reshape(-1, 3), "vert_key": np.asarray(mesh["vert_key"])[used],
            "triangles": tri}


# ---- scenes
def look_at(position, target=(0.0, 0.0, 0.0)):
    """c2w fp32 [3,4] of a camera at `position` looking at `target`: columns right, up, -forward, position (the camera looks
    along its -z; x right, y up).  World up is z, or y when the view direction is along z."""
    pos, tgt = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = (tgt - pos) / np.linalg.norm(tgt - pos)
    up = np.array([0.0, 0.0, 1.0]) if abs(f[2]) < 0.99 else np.array([0.0, 1.0, 0.0])
    right = np.cross(f, up)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(right, f), -f, pos], axis=1).astype(F32)


def view_directions(n_views):
    """6: the axes; 14: plus the 8 cube diagonals; 26: plus the 12 edge midpoints.  Unit vectors, float64 [n,3]."""
    d = [v for v in np.ndindex(3, 3, 3)]
    d = np.array(d, dtype=np.float64) - 1.0
    order = np.abs(d).sum(1)
    pick = {6: order == 1, 14: (order == 1) | (order == 3), 26: order >= 1}[n_views]
    d = d[pick]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def pixel_rays(c2w, height, width, fx, fy, cx, cy):
    """The header's ray convention in fp64: -> (origin [3], unit directions [H*W,3]), row-major."""
    m = np.asarray(c2w, dtype=np.float64)
    y, x = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    v = np.stack([(x + 0.5 - cx) / fx, -(y + 0.5 - cy) / fy, -np.ones_like(x, dtype=np.float64)], axis=-1).reshape(-1, 3)
    d = v @ m[:, :3].T
    return m[:, 3], d / np.linalg.norm(d, axis=1, keepdims=True)


def sphere_depth(c2w, height, width, fx, fy, cx, cy, radius, far, centre=(0.0, 0.0, 0.0)):
    """Median depth of an opaque sphere: the distance to the first intersection, `far` for a ray that misses.  fp32 [H*W]."""
    o, d = pixel_rays(c2w, height, width, fx, fy, cx, cy)
    oc = o - np.asarray(centre, dtype=np.float64)
    b = d @ oc
    disc = b * b - (oc @ oc - radius * radius)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    return np.where((disc > 0) & (t > 0), t, far).astype(F32)
