"""rsn_ssim's reference and cases: the per-position SSIM term of data_reference.ssim (torchmetrics' definition: Gaussian 11, sigma 1.5,
k1 0.01, k2 0.03, L from the images unless given) in float64 and, as a plain restatement of the same formula, in float32 -- the
reference project's own precision, not an emulation of the kernel's operation order.  The case table puts the last window position on,
before and after the seams of the kernel's 32 x 16 tiles, and holds the image classes of a rendered view: exactly constant
backgrounds, a constant target, values at the ends of [0, 1], single-pixel differences around a seam, differing channels, scaled
images and a caller-chosen data range.

The bound of a case is  FACTOR x |ssim_mean(float32) - ssim_mean(float64)| + 2^-24  (FACTOR = 4 as in field_maths_reference; 2^-24:
the rounding of the fp32 output).  Nothing in it comes from a run of the kernel.

The building blocks (window_moments with per-position tap masks, ssim_terms) are what tests/test_ssim_cpu.py states its wrong kernels
with."""
import functools

import numpy as np

from tests.field_maths_reference import FACTOR

K = 11                      # window
HALO = K - 1
TX, TY = 32, 16             # rsn_ssim_tile_kernel: window positions per workgroup
OUT_ROUNDING = 2.0 ** -24   # the fp32 output of a mean in [-1, 1]
BOUND_CAP = 1e-4


def taps(dtype=np.float64, k=K, sigma=1.5):
    """torchmetrics' _gaussian: exp(-(t / sigma)^2 / 2), t = -5 .. 5, normalised; every operation in `dtype`."""
    dt = np.dtype(dtype).type
    t = np.arange(k, dtype=dtype) - dt((k - 1) / 2)
    q = t / dt(sigma)
    g = np.exp(-(q * q) / dt(2))
    return (g / g.sum(dtype=dtype)).astype(dtype)


def window_moments(p, t, g, mask_x=None, mask_y=None):
    """The five filtered moments (p, t, p^2, t^2, pt) at every full-window position, [5][H-10, W-10, C], separable: along x, then
    along y.  mask_x [W-10, 11] / mask_y [H-10, 11]: the weight of tap k at position px / py is g[k] * mask[px, k] (a tap the kernel
    would read as zero from its LDS patch); None: all ones."""
    H, W = p.shape[:2]
    ny, nx = H - HALO, W - HALO

    def filt(a):
        h = 0
        for k in range(K):
            w = g[k] if mask_x is None else (g[k] * mask_x[:, k])[None, :, None]
            h = h + w * a[:, k:k + nx]
        v = 0
        for k in range(K):
            w = g[k] if mask_y is None else (g[k] * mask_y[:, k])[:, None, None]
            v = v + w * h[k:k + ny]
        return v

    return filt(p), filt(t), filt(p * p), filt(t * t), filt(p * t)


def ssim_terms(m, c1, c2):
    mp, mt, epp, ett, ept = m
    spp = epp - mp * mp
    stt = ett - mt * mt
    spt = ept - mp * mt
    return ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))


def data_range_of(pred, target):
    return max(pred.max() - pred.min(), target.max() - target.min())


def constants(L, dtype):
    dt = np.dtype(dtype).type
    L = dt(L)
    return (dt(0.01) * L) * (dt(0.01) * L), (dt(0.03) * L) * (dt(0.03) * L)


def ssim_map(pred, target, data_range=None, dtype=np.float64, g=None, mask_x=None, mask_y=None):
    """-> [H-10, W-10, 3] in `dtype`: the SSIM term per window position (top-left pixel) and channel."""
    p = np.asarray(pred, dtype=dtype)
    t = np.asarray(target, dtype=dtype)
    assert p.shape == t.shape and p.ndim == 3 and p.shape[0] >= K and p.shape[1] >= K
    L = data_range_of(p, t) if data_range is None else data_range
    c1, c2 = constants(L, dtype)
    g = taps(dtype) if g is None else np.asarray(g, dtype=dtype)
    s = ssim_terms(window_moments(p, t, g, mask_x, mask_y), c1, c2)
    assert s.dtype == np.dtype(dtype)
    return s


def ssim_mean(pred, target, data_range=None, dtype=np.float64):
    s = ssim_map(pred, target, data_range, dtype)
    return float(s.mean(dtype=dtype))


def grid(H, W):
    """Workgroups of rsn_ssim_tile_kernel along (y, x)."""
    return -(-(H - HALO) // TY), -(-(W - HALO) // TX)


# ---------------------------------------------------------------------------------------------- shapes
# (ny, nx) = (H - 10, W - 10): the last position on, one before and one after a seam, one partial tile, a full tile plus one row or
# column, three tiles.  Every value of {1, 15, 16, 17, 33} x {1, 31, 32, 33, 65} at least once and the four corners.
SEAM_SHAPES = ((1, 1), (1, 65), (33, 1), (33, 65), (16, 32), (17, 33), (15, 31), (15, 33), (17, 31), (16, 65), (33, 32), (1, 32),
               (16, 1))
BIG = (16 * 17 + 1, 32 * 16 + 1)  # 283 x 523 pixels, 18 x 17 = 306 workgroups: the reduce kernel's stride loop, all four waves
TWO_TILES = (17, 33)              # one full tile plus a single row and column
THREE_TILES = (33, 65)
SCALES = (4.0, 0.25)


def _hw(shape):
    return shape[0] + HALO, shape[1] + HALO


def _tag(shape):
    return f"{shape[0]}x{shape[1]}"


def _rng(cls, shape):
    # a stable seed per (class, shape): str hashes are salted per process, so spell the class out as bytes
    return np.random.default_rng([int.from_bytes(cls.encode()[:8].ljust(8, b"\0"), "little"), shape[0], shape[1]])


def _smooth(H, W, lo=0.4, amp=0.3):
    yy, xx = np.meshgrid(np.arange(H) / 16.0, np.arange(W) / 16.0, indexing="ij")
    return np.stack([lo + amp * np.sin(2.1 * xx + 1.3 * yy + 1.7 * k) for k in range(3)], -1).astype(np.float32)


def _random(shape):
    H, W = _hw(shape)
    r = _rng("random", shape)
    return r.random((H, W, 3)).astype(np.float32), r.random((H, W, 3)).astype(np.float32)


def _noisy(shape):
    H, W = _hw(shape)
    r = _rng("noisy", shape)
    a = r.random((H, W, 3)).astype(np.float32)
    return np.clip(a + 0.1 * r.normal(size=a.shape), 0, 1).astype(np.float32), a


def _render_like(shape):
    """An exactly white background, a shaded disc across the tile seams; the prediction differs inside the disc only."""
    H, W = _hw(shape)
    r = _rng("render", shape)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cy, cx, rad = 0.5 * H + 1.5, 0.5 * W - 2.5, 0.36 * min(H, W)
    dy, dx = (yy - cy) / rad, (xx - cx) / rad
    inside = dy * dy + dx * dx < 1.0
    z = np.sqrt(np.clip(1.0 - dy * dy - dx * dx, 0, None))
    shade = 0.25 + 0.75 * np.clip(0.5 * dx - 0.6 * dy + 0.62 * z, 0, None)
    target = np.where(inside[..., None], shade[..., None] * np.array([0.85, 0.35, 0.25]), 1.0).astype(np.float32)
    noise = (0.03 * r.normal(size=target.shape)).astype(np.float32)
    pred = np.where(inside[..., None], np.clip(target + noise, 0, 1), target).astype(np.float32)
    assert inside.any() and not inside.all() and np.array_equal(pred[~inside], target[~inside]) and (target[~inside] == 1.0).all()
    return pred, target


def _white_target(shape):
    H, W = _hw(shape)
    r = _rng("white", shape)
    target = np.ones((H, W, 3), np.float32)
    pred = (1.0 - np.abs(0.05 * r.normal(size=target.shape))).astype(np.float32)
    return pred, target


def _ends(shape):
    """Exact zeros and ones in 5 x 7 blocks against their blurred copy."""
    H, W = _hw(shape)
    yy, xx = np.meshgrid(np.arange(H) // 5, np.arange(W) // 7, indexing="ij")
    target = np.repeat((((yy + xx) % 2) == 0).astype(np.float32)[..., None], 3, -1)
    target[..., 1] = 1.0 - target[..., 1]
    pad = np.pad(target.astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    blur = sum(pad[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    return blur.astype(np.float32), target


def _impulse(shape, y, x):
    H, W = _hw(shape)
    assert 0 <= y < H and 0 <= x < W
    target = _smooth(H, W)
    pred = target.copy()
    pred[y, x] += np.float32(0.25)
    return pred, target


def _channels(shape):
    """Channel 0: unrelated noise, channel 1: bit-equal, channel 2: the target plus noise."""
    H, W = _hw(shape)
    r = _rng("channels", shape)
    target = _smooth(H, W)
    target[..., 0] = r.random((H, W)).astype(np.float32)
    pred = target.copy()
    pred[..., 0] = r.random((H, W)).astype(np.float32)
    pred[..., 2] = np.clip(pred[..., 2] + 0.05 * r.normal(size=(H, W)), 0, 1).astype(np.float32)
    return pred, target


def _half_range(shape):
    """Values in [0.25, 0.75], both ends present in both images: the images' own range is exactly 0.5."""
    H, W = _hw(shape)
    r = _rng("half", shape)
    a = (0.25 + 0.5 * r.random((H, W, 3))).astype(np.float32)
    b = np.clip(a + 0.05 * r.normal(size=a.shape), 0.25, 0.75).astype(np.float32)
    for im in (a, b):
        im[0, 0, 0], im[-1, -1, 2] = 0.25, 0.75
    return b, a


def _scaled(maker, shape, k):
    p, t = maker(shape)
    return (np.float32(k) * p), (np.float32(k) * t)


def impulse_pixels(shape):
    """Pixels of interest of a shape with at least two tiles per axis -> {label: (y, x)}: the image corners and, relative to each tile
    origin that has a next tile in both axes, (15, 31): the last pixel whose windows all lie in that tile, (16, 32): the first pixel
    of the next tile's own area, (25, 41) and (26, 42): the two ends of the halo."""
    H, W = _hw(shape)
    gy, gx = grid(H, W)
    assert gy >= 2 and gx >= 2
    px = {"corner00": (0, 0), "cornerHW": (H - 1, W - 1)}
    for ty, tx in ((0, 0), (1, 1)):
        if ty + 1 >= gy or tx + 1 >= gx:
            continue
        for oy, ox in ((15, 31), (16, 32), (25, 41), (26, 42)):
            y, x = ty * TY + oy, tx * TX + ox
            if y < H and x < W:
                px[f"t{ty}{tx}p{oy}_{ox}"] = (y, x)
    return px


BIG_IMPULSE = (16 * TY + 25, 5 * TX + 41)  # the halo's far end of workgroup 16 * 17 + 5 = 277, beyond the reduce kernel's first trip


def _table():
    t = {}

    def add(name, maker, *args, data_range=None, cls=None, shape=None):
        assert name not in t
        t[name] = {"make": functools.partial(maker, *args), "data_range": data_range, "class": cls or name.split("_")[0],
                   "shape": shape or args[0]}

    for s in SEAM_SHAPES + (BIG,):
        add(f"random_{_tag(s)}", _random, s)
        add(f"noisy_{_tag(s)}", _noisy, s)
    for s in ((16, 32), TWO_TILES, (15, 33), THREE_TILES, BIG):
        add(f"render_like_{_tag(s)}", _render_like, s, cls="render_like")
    for s in ((1, 65), (33, 1), TWO_TILES, THREE_TILES, BIG):
        add(f"white_target_{_tag(s)}", _white_target, s, cls="white_target")
    for s in ((15, 31), TWO_TILES, THREE_TILES):
        add(f"ends_{_tag(s)}", _ends, s)
    for s in (TWO_TILES, THREE_TILES):
        for label, (y, x) in impulse_pixels(s).items():
            add(f"impulse_{_tag(s)}_{label}", _impulse, s, y, x)
        add(f"channels_{_tag(s)}", _channels, s)
    add(f"impulse_{_tag(BIG)}_wg277", _impulse, BIG, *BIG_IMPULSE)
    for k in SCALES:
        add(f"scaled_random_{_tag(TWO_TILES)}_x{k:g}", _scaled, _random, TWO_TILES, k, shape=TWO_TILES)
        add(f"scaled_render_like_{_tag(TWO_TILES)}_x{k:g}", _scaled, _render_like, TWO_TILES, k, shape=TWO_TILES)
    for s in (TWO_TILES, THREE_TILES):
        add(f"explicit_range1_{_tag(s)}", _half_range, s, data_range=1.0, cls="explicit")
    return t


CASES = _table()
CLASSES = tuple(dict.fromkeys(c["class"] for c in CASES.values()))


def names(cls=None):
    return [n for n, c in CASES.items() if cls is None or c["class"] == cls]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (pred, target, data_range or None); float32 [H, W, 3], read-only."""
    c = CASES[name]
    p, t = c["make"]()
    H, W = _hw(c["shape"])
    assert p.shape == t.shape == (H, W, 3) and p.dtype == t.dtype == np.float32
    assert data_range_of(p.astype(np.float64), t.astype(np.float64)) > 0  # constant against constant is outside the definition
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t, c["data_range"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> dict: ref (float64 mean), f32 (the float32 restatement's mean), f32_err, bound, count (positions x channels)."""
    p, t, L = case(name)
    ref = ssim_mean(p, t, L, np.float64)
    f32 = ssim_mean(p, t, L, np.float32)
    return {"ref": ref, "f32": f32, "f32_err": abs(f32 - ref), "bound": bound(f32, ref), "count": 3 * (p.shape[0] - HALO) * (p.shape[1] - HALO)}


def bound(f32, ref):
    return FACTOR * abs(f32 - ref) + OUT_ROUNDING
