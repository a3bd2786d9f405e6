"""fp64 restatement of the per-sample occupancy rules of include/rsn.h (rsn_occupancy_compact_samples / rsn_scatter_level), on top
of tests/occupancy_reference.py: a sample is the sub-segment [t_i, t_i+1] of its ray, so the two predicates of the sandwich are
hits_shrunk / hits_grown of that file on the rays repeated once per sample.

    make_bins             sorted bin edges in [near, far] (whatever near and far are: a non-finite or reversed pair gives samples
                          that cannot be reasoned about, which must be live)
    sample_predicates     must / may / invalid, [R,S] each
    footprint             rule (b): t_i+1 * |d| * sqrt(pixel_area / pi) > max_radius, fp64 on the fp32 inputs
    brute_force           point sampling of every sub-segment: does a point lie in an occupied cell (or an end point outside the box)
    level_case            random members of a level for the scatter test
"""
import numpy as np

from tests import occupancy_reference as ref

SHAPES = ((1, 1), (63, 1), (21, 3), (64, 1), (1, 64), (65, 1), (3075, 1), (1025, 3), (1100, 64))  # (R, S): R*S = 1 63 64 65 3075 70400
MEMBERS = (("sigma", 1), ("color", 3), ("pred_normals", 3), ("n_dot_d", 1), ("diff", 3), ("tint", 3), ("roughness", 1),
           ("raw_density", 1), ("raw_roughness", 1))


def make_bins(near, far, S, seed):
    """near / far fp32 [R] -> fp32 [R,S+1]: near + (far - near) * u with u sorted, u_0 = 0 and u_S = 1; computed in fp32 and then
    sorted again along the ray when all of it is finite and far >= near, so that rounding cannot reverse a pair of edges."""
    rng = np.random.default_rng(6000 + seed)
    R = len(near)
    u = np.sort(rng.uniform(size=(R, S + 1)), axis=1).astype(np.float32)
    u[:, 0], u[:, -1] = 0.0, 1.0
    near, far = np.asarray(near, np.float32)[:, None], np.asarray(far, np.float32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        bins = (near + (far - near) * u).astype(np.float32)
        good = np.isfinite(bins).all(axis=1) & (far[:, 0] >= near[:, 0])
    bins[good] = np.sort(bins[good], axis=1)
    return np.ascontiguousarray(bins)


def expand(o, d, bins):
    """-> the rays repeated once per sample, and the samples' (t_i, t_i+1): [R*S,3], [R*S,3], [R*S], [R*S]."""
    S = bins.shape[1] - 1
    return (np.repeat(o, S, axis=0), np.repeat(d, S, axis=0), np.ascontiguousarray(bins[:, :-1]).reshape(-1),
            np.ascontiguousarray(bins[:, 1:]).reshape(-1))


def sample_predicates(o, d, bins, occ, origin, spacing, outside, subset=None):
    """-> must, may, invalid (bool, [R*S] or [len(subset)]): the samples that have to be live, that may be, and that cannot be
    reasoned about (these are in both)."""
    oo, dd, t0, t1 = expand(o, d, bins)
    if subset is not None:
        oo, dd, t0, t1 = oo[subset], dd[subset], t0[subset], t1[subset]
    return (ref.hits_shrunk(oo, dd, t0, t1, occ, origin, spacing, outside), ref.hits_grown(oo, dd, t0, t1, occ, origin, spacing, outside),
            ref.invalid_rays(oo, dd, t0, t1))


def footprint(d, pixel_area, bins, max_radius):
    """Rules (b) and (c) -> bool [R,S]."""
    d64, pa = np.asarray(d, np.float64), np.asarray(pixel_area, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        radius = np.asarray(bins, np.float64)[:, 1:] * np.sqrt((d64 * d64).sum(axis=1))[:, None] * np.sqrt(pa / np.pi)[:, None]
        return (radius > np.float64(max_radius)) | ~np.isfinite(pa)[:, None]


def brute_force(o, d, bins, occ, origin, spacing, outside, K):
    """K + 1 evenly spaced points of every sub-segment (both ends among them), fp64 -> bool [R*S]: a point lies in a closed occupied
    cell, or (outside) an end point lies outside the box.  Samples must be valid."""
    oo, dd, t0, t1 = (np.asarray(a, np.float64) for a in expand(o, d, bins))
    origin, spacing = np.asarray(origin, np.float64), np.asarray(spacing, np.float64)
    cz, cy, cx = occ.shape
    cells = np.array([cx, cy, cz])
    hit = np.zeros(len(t0), dtype=bool)
    for k in range(K + 1):
        t = t0 + (t1 - t0) * (k / K)
        g = (oo + t[:, None] * dd - origin) / spacing  # grid coordinates
        inside = ((g >= 0.0) & (g <= cells)).all(axis=1)
        if outside and k in (0, K):
            hit |= ~inside
        # a point on a face belongs to both cells: try the cell below and the cell above every coordinate that is an integer
        lo = np.clip(np.floor(g).astype(np.int64), 0, cells - 1)
        up = np.clip(np.ceil(g).astype(np.int64) - 1, 0, cells - 1)
        for ix in (lo[:, 0], up[:, 0]):
            for iy in (lo[:, 1], up[:, 1]):
                for iz in (lo[:, 2], up[:, 2]):
                    hit |= inside & occ[iz, iy, ix]
    return hit


def level_case(n, seed):
    """Random members of a level with n rows -> {name: fp32 [n] or [n,3]}."""
    rng = np.random.default_rng(7000 + seed)
    return {name: rng.normal(size=(n,) if row == 1 else (n, row)).astype(np.float32) for name, row in MEMBERS}
