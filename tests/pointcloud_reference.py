"""Numpy restatement of the point-cloud contract of include/rsn.h (rsn_pointcloud_mark / rsn_pointcloud_select) -- fp32, every
step one numpy fp32 operation in the header's order, so that the device result can be compared bit for bit.  Written from the
header's text, not from the kernels.  The rays are an input: the GPU tests pass the ones render.camera_rays returns (the device
function the calls run), the CPU tests analytic ones.  Also a reader for exactly what pointcloud.write_ply_points promises."""
import numpy as np

F32 = np.float32
NO_OWNER = 0x7FFFFFFF


def candidates(rays_o, rays_d, depth, acc, height, width, dims, origin, spacing, min_accumulation, edge):
    """rays_o / rays_d: fp32 [n, H*W, 3]; depth: [n, H*W]; acc: [n, H*W] or None; dims = (nx, ny, nz) cells.
    -> (candidate bool [n, H*W], point fp32 [n, H*W, 3], flat cell int64 [n, H*W] (-1 where the pixel is no candidate))."""
    H, W = int(height), int(width)
    o = np.asarray(rays_o, dtype=F32).reshape(-1, H * W, 3)
    d = np.asarray(rays_d, dtype=F32).reshape(-1, H * W, 3)
    n = o.shape[0]
    D = np.asarray(depth, dtype=F32).reshape(n, H, W)
    org, spc = np.asarray(origin, dtype=F32), np.asarray(spacing, dtype=F32)
    min_accumulation, edge = F32(min_accumulation), F32(edge)
    with np.errstate(all="ignore"):
        ok = np.isfinite(D) & (D > 0)                                                        # rule 1
        if acc is not None:
            ok &= np.asarray(acc, dtype=F32).reshape(n, H, W) >= min_accumulation            # rule 2: a NaN fails
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):                                    # rule 3
            Dn = np.full_like(D, np.nan)  # outside the image: no neighbour
            ys, yd = (slice(0, H - 1), slice(1, H)) if dy < 0 else (slice(1, H), slice(0, H - 1)) if dy > 0 else (slice(None),) * 2
            xs, xd = (slice(0, W - 1), slice(1, W)) if dx < 0 else (slice(1, W), slice(0, W - 1)) if dx > 0 else (slice(None),) * 2
            Dn[:, yd, xd] = D[:, ys, xs]
            diff, lim = np.abs(D - Dn), edge * np.minimum(D, Dn)
            assert diff.dtype == F32 and lim.dtype == F32
            ok &= ~(np.isfinite(Dn) & (diff > lim))  # a NaN product compares false
        Dp = D.reshape(n, H * W)
        pos = np.empty((n, H * W, 3), dtype=F32)
        idx = []
        inside = np.ones((n, H * W), dtype=bool)
        for a in range(3):                                                                   # rule 4
            t = Dp * d[:, :, a]
            pos[:, :, a] = o[:, :, a] + t
            q = (pos[:, :, a] - org[a]) / spc[a]
            assert t.dtype == F32 and q.dtype == F32
            inside &= (q >= 0) & (q < F32(dims[a]))  # a NaN fails
            idx.append(np.where(inside, np.floor(q), 0).astype(np.int64))
    cand = ok.reshape(n, H * W) & inside
    cell = np.where(cand, (idx[2] * int(dims[1]) + idx[1]) * int(dims[0]) + idx[0], -1)
    return cand, pos, cell


def global_index(n_views, height, width, view0):
    return (int(view0) * int(height) * int(width) + np.arange(int(n_views) * int(height) * int(width), dtype=np.int64)).reshape(n_views, -1)


def mark(owner, cand, cell, height, width, view0):
    """owner: int32 [nz, ny, nx] (or None: no thinning, returns None) -> the new owner; the input is not modified."""
    if owner is None:
        return None
    out = np.array(owner, dtype=np.int32, copy=True)
    g = global_index(cand.shape[0], height, width, view0)
    np.minimum.at(out.reshape(-1), cell[cand], g[cand].astype(np.int32))
    return out


def select(owner, cand, pos, cell, height, width, view0):
    """-> (n_points, pixel_index int32 [P] ascending, positions fp32 [P,3]) of the kept pixels of this call."""
    g = global_index(cand.shape[0], height, width, view0)
    kept = cand.copy()
    if owner is not None:
        kept[cand] = np.asarray(owner).reshape(-1)[cell[cand]] == g[cand]
    return int(kept.sum()), g[kept].astype(np.int32), pos[kept]


def mark_select(owner, rays_o, rays_d, depth, acc, height, width, view0, dims, origin, spacing, min_accumulation, edge):
    """One mark + select pair -> (owner after mark, n_points, pixel_index, positions, candidate mask, cells)."""
    cand, pos, cell = candidates(rays_o, rays_d, depth, acc, height, width, dims, origin, spacing, min_accumulation, edge)
    owner = mark(owner, cand, cell, height, width, view0)
    return (owner,) + select(owner, cand, pos, cell, height, width, view0) + (cand, cell)


def new_owner(dims):
    return np.full((int(dims[2]), int(dims[1]), int(dims[0])), NO_OWNER, dtype=np.int32)


def parse_ply_points(path):
    """A reader for exactly what write_ply_points promises: -> (vertex dict of arrays, header lines)."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").strip().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    elements = [ln.split() for ln in lines if ln.startswith("element")]
    assert len(elements) == 1 and elements[0][1] == "vertex", elements  # no face element
    kinds = {"float": "<f4", "uchar": "u1"}
    vdt = np.dtype([(w[2], kinds[w[1]]) for w in (ln.split() for ln in lines if ln.startswith("property"))])
    nv = int(elements[0][2])
    assert end + nv * vdt.itemsize == len(blob)
    vert = np.frombuffer(blob, dtype=vdt, count=nv, offset=end)
    return {n: vert[n] for n in vdt.names}, lines
