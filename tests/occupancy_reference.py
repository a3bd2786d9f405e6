"""fp64 restatement of the occupancy calls of include/rsn.h, for the CPU and GPU tests.

    build_cells / pack_bits      the build rule, stated literally over vertices, and the bit layout
    hits_shrunk / hits_grown     the two predicates of the sandwich the culling kernel has to lie between
    expected_index               the permutation that belongs to a vector of flags
    grid_case / ray_cases / face_plane_rays   the inputs the tests share

The sandwich.  The kernel may decide either way inside a band of BAND = 1e-3 of a cell around the cell faces.  So the occupied
region is stated twice: SHRUNK (every occupied cell shrunk by BAND of a cell on every side; with outside_occupied the outside of
the box shrunk as well, i.e. the box grown by BAND) and GROWN (the cells grown, the box shrunk).  A segment that meets the shrunk
region must be flagged; a segment that does not meet the grown region must be culled; in between either answer is right.  A ray
with a non-finite component or far < near meets both by definition.  Segments are tested against boxes with the slab method in
fp64 on the fp32 inputs; the outside of a (convex) box is met exactly when one of the two end points lies outside it.
"""
import numpy as np

BAND = 1e-3
DIMS = ((2, 2, 2), (12, 7, 5), (33, 34, 3))
RAY_COUNTS = (1, 63, 64, 65, 1025)


# ------------------------------------------------------------------------------------------------ build
def build_cells(vol, threshold, dilate):
    """vol [nz, ny, nx] -> bool [nz-1, ny-1, nx-1]: cell (i, j, k) is occupied iff some vertex (i', j', k') of the grid has
    not (vol < threshold), i - dilate <= i' <= i + 1 + dilate and likewise for j, k."""
    vol = np.asarray(vol, dtype=np.float32)
    nz, ny, nx = vol.shape
    with np.errstate(invalid="ignore"):
        solid = ~(vol < np.float32(threshold))
    occ = np.zeros((nz - 1, ny - 1, nx - 1), dtype=bool)
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                occ[k, j, i] = solid[max(k - dilate, 0):min(k + 1 + dilate, nz - 1) + 1,
                                     max(j - dilate, 0):min(j + 1 + dilate, ny - 1) + 1,
                                     max(i - dilate, 0):min(i + 1 + dilate, nx - 1) + 1].any()
    return occ


def n_words(dims):
    nx, ny, nz = dims
    return ((nx - 1) * (ny - 1) * (nz - 1) + 31) // 32


def pack_bits(occ):
    """bool [cz, cy, cx] -> uint32 words: cell c = (k*cy + j)*cx + i is bit c % 32 of word c / 32; pad bits 0."""
    flat = np.asarray(occ, dtype=bool).reshape(-1)
    padded = np.zeros((len(flat) + 31) // 32 * 32, dtype=np.uint64)
    padded[:len(flat)] = flat
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ cull
def invalid_rays(o, d, near, far):
    o, d, near, far = (np.asarray(a, dtype=np.float64) for a in (o, d, near, far))
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(near) & np.isfinite(far)) | (far < near)


def _segment_meets_boxes(o, d, near, far, lo, hi):
    """Closed segments [R] against closed boxes [n,3] -> bool [R]: any box met.  Slab method, fp64; rays must be finite."""
    R = len(o)
    out = np.zeros(R, dtype=bool)
    if len(lo) == 0 or R == 0:
        return out
    for r0 in range(0, R, 256):
        oo, dd = o[r0:r0 + 256, None, :], d[r0:r0 + 256, None, :]
        par = dd == 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (lo[None] - oo) / dd, (hi[None] - oo) / dd
        tlo = np.where(par, -np.inf, np.minimum(ta, tb))
        thi = np.where(par, np.inf, np.maximum(ta, tb))
        inside = np.where(par, (oo >= lo[None]) & (oo <= hi[None]), True).all(axis=2)
        t0 = np.maximum(tlo.max(axis=2), near[r0:r0 + 256, None])
        t1 = np.minimum(thi.min(axis=2), far[r0:r0 + 256, None])
        out[r0:r0 + 256] = (inside & (t0 <= t1)).any(axis=1)
    return out


def _predicate(o, d, near, far, occ, origin, spacing, outside_occupied, delta):
    """delta > 0: the occupied region shrunk by delta cells; delta < 0: grown."""
    o, d, near, far = (np.asarray(a, dtype=np.float64) for a in (o, d, near, far))
    origin, spacing = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    bad = invalid_rays(o, d, near, far)
    oo, dd, nn, ff = (np.where(bad.reshape(-1, *[1] * (a.ndim - 1)), 0.0, a) for a in (o, d, near, far))
    kji = np.argwhere(occ)
    ijk = kji[:, ::-1].astype(np.float64)
    hit = _segment_meets_boxes(oo, dd, nn, ff, origin + spacing * (ijk + delta), origin + spacing * (ijk + 1.0 - delta))
    if outside_occupied:
        cells = np.asarray(occ.shape[::-1], dtype=np.float64)
        blo, bhi = origin + spacing * (0.0 - delta), origin + spacing * (cells + delta)  # the OUTSIDE shrinks: the box grows
        for p in (oo + nn[:, None] * dd, oo + ff[:, None] * dd):
            hit |= ((p < blo) | (p > bhi)).any(axis=1)
    return hit | bad


def hits_shrunk(o, d, near, far, occ, origin, spacing, outside_occupied):
    """Rays that MUST be flagged."""
    return _predicate(o, d, near, far, occ, origin, spacing, outside_occupied, BAND)


def hits_grown(o, d, near, far, occ, origin, spacing, outside_occupied):
    """Rays that MAY be flagged; every other ray must be culled."""
    return _predicate(o, d, near, far, occ, origin, spacing, outside_occupied, -BAND)


def expected_index(hit):
    hit = np.asarray(hit).astype(bool)
    return np.concatenate([np.flatnonzero(hit), np.flatnonzero(~hit)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ shared inputs
def grid_frame(dims, seed):
    """An off-centre box with unequal spacings -> origin [3], spacing [3] (fp32)."""
    rng = np.random.default_rng(1000 + seed)
    spacing = rng.uniform(0.05, 0.3, size=3).astype(np.float32)
    origin = rng.uniform(-1.0, 0.5, size=3).astype(np.float32)
    return origin, spacing


def grid_case(dims, share, seed):
    """-> occ bool [cz, cy, cx] with about `share` of the cells occupied (at least one, and at least one free when there are two)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(2000 + seed)
    occ = rng.uniform(size=(nz - 1, ny - 1, nx - 1)) < share
    flat = occ.reshape(-1)
    flat[rng.integers(len(flat))] = True
    if len(flat) > 1 and flat.all():
        flat[0] = False
    return occ


def build_volume(dims, seed, threshold=0.5):
    """A random volume with entries equal to the threshold, NaN and +-inf."""
    nx, ny, nz = dims
    rng = np.random.default_rng(3000 + seed)
    vol = rng.uniform(0.0, 0.62, size=(nz, ny, nx)).astype(np.float32)  # about a fifth of the vertices solid
    flat = vol.reshape(-1)
    n = len(flat)
    each = max(1, n // 40)
    where = rng.permutation(n)  # distinct places: the smallest grid has eight vertices for five special values
    for v, value in enumerate((threshold, np.nan, np.inf, -np.inf, np.nextafter(np.float32(threshold), np.float32(0)))):
        flat[where[v * each:(v + 1) * each]] = value
    return vol


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


N_FAMILIES = 7


def ray_cases(dims, origin, spacing, n, seed):
    """n rays, ray r of family r % 7: 0 through the box from outside, 1 origin inside, 2 missing the box, 3 one or two zero direction
    components (+0.0 and -0.0), 4 directions of length 0.1 and 10, 5 windows that end before the box, begin after it or lie inside
    one cell, 6 non-finite inputs and far < near.  -> o [n,3], d [n,3], near [n], far [n] (fp32), family [n]."""
    rng = np.random.default_rng(4000 + seed)
    origin, spacing = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    cells = np.asarray(dims, dtype=np.float64) - 1.0
    lo, hi = origin, origin + spacing * cells
    centre, diag = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    fam = (np.arange(n) + seed) % N_FAMILIES
    o = centre + (1.0 + rng.uniform(0.0, 1.0, size=(n, 1))) * diag * _unit(rng, n)  # outside the box
    target = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    d = target - o
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    near, far = np.zeros(n), 2.0 * dist
    inside = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    for r in range(n):
        f = fam[r]
        if f == 1:
            o[r], d[r], far[r] = inside[r], _unit(rng, 1)[0], rng.uniform(0.1, 1.0) * diag
        elif f == 2:
            d[r] = (o[r] - centre) / np.linalg.norm(o[r] - centre) if rng.uniform() < 0.5 else np.cross(o[r] - centre, _unit(rng, 1)[0])
            d[r] /= np.linalg.norm(d[r])
        elif f == 3:
            o[r] = inside[r]
            zero = rng.permutation(3)[:rng.integers(1, 3)]
            d[r] = _unit(rng, 1)[0]
            d[r, zero] = rng.choice([0.0, -0.0], size=len(zero))
            d[r] /= np.linalg.norm(d[r])
            if rng.uniform() < 0.5:  # start outside: back the origin off along the ray
                o[r] = o[r] - d[r] * 2.0 * diag
                far[r] = 4.0 * diag
            else:
                far[r] = diag
        elif f == 4:
            s = 0.1 if rng.uniform() < 0.5 else 10.0
            d[r] *= s
            far[r] /= s
        elif f == 5:
            kind = rng.integers(3)
            if kind == 0:
                far[r] = 0.4 * (dist[r] - 0.5 * diag)  # ends well before the box (the origin is at least a diagonal away)
            elif kind == 1:
                near[r], far[r] = dist[r] + 1.1 * diag, dist[r] + 2.0 * diag
            else:  # inside one cell, away from its faces
                cell = np.floor(rng.uniform(size=3) * cells)
                o[r] = lo + spacing * (cell + rng.uniform(0.3, 0.7, size=3))
                d[r] = _unit(rng, 1)[0]
                near[r], far[r] = 0.0, 0.2 * spacing.min()
        elif f == 6:
            kind = rng.integers(5)
            bad = rng.choice([np.nan, np.inf, -np.inf])
            if kind == 0:
                o[r, rng.integers(3)] = bad
            elif kind == 1:
                d[r, rng.integers(3)] = bad
            elif kind == 2:
                near[r] = bad
            elif kind == 3:
                far[r] = bad
            else:
                near[r], far[r] = far[r], 0.5 * far[r] - 1.0
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return f32(o), f32(d), f32(near), f32(far), fam


def face_plane_rays(dims, origin, spacing, n, seed):
    """Rays that lie exactly in cell-face planes: one coordinate of the origin is a vertex coordinate in fp32 and the direction
    has a zero there.  Either answer is right for them: only determinism and the index property are checked."""
    rng = np.random.default_rng(5000 + seed)
    origin, spacing = np.asarray(origin, dtype=np.float32), np.asarray(spacing, dtype=np.float32)
    cells = np.asarray(dims) - 1
    o = (origin + spacing * (rng.uniform(size=(n, 3)) * cells).astype(np.float32)).astype(np.float32)
    d = _unit(rng, n).astype(np.float32)
    for r in range(n):
        a = rng.integers(3)
        o[r, a] = origin[a] + spacing[a] * np.float32(rng.integers(0, cells[a] + 1))
        d[r, a] = rng.choice([0.0, -0.0])
    return o, d, np.zeros(n, dtype=np.float32), np.full(n, 5.0, dtype=np.float32)
