"""Host restatements (numpy) of include/rsn.h, "captures: masks and fisheye lenses", written from the recipes there and not from the
kernels or the loader:

    fisheye_forward / fisheye_inverse   OpenCV's equidistant model in float64 and its inverse, bisected to the last bit
    rays                                origins, directions and pixel_area of a 9- or 12-column row by the literal definition, float64
    rays_f32                            the kernel recipe with its float32 steps in float32; used ONLY to size the GPU tests' bounds
    level_liveness / live_lists         a level pixel is live when all the pixels under it are; the lists are numpy.flatnonzero
    sample_through_lists                the level + pixel draw of rsn_sample_capture_rays_live on tests/data_reference.philox4x32_10
    the masks of the GPU tests, and writers of masked / fisheye / downscaled captures on disk
"""
import json
import math
import os

import numpy as np

from tests import capture_reference as cref
from tests.data_reference import philox4x32_10

MILD = (-0.03, 0.006, -0.001, 0.0002)  # k1 k2 k3 k4


def fisheye_row(width=52, height=36, coeffs=MILD, corner_theta_d=1.4, cx=None, cy=None):
    """A 12-column fisheye row whose far corner pixel centre lies at theta_d = corner_theta_d; fx != fy, principal point off centre."""
    cx = width / 2.0 - 0.7 if cx is None else cx
    cy = height / 2.0 + 0.4 if cy is None else cy
    ax, ay = max(cx - 0.5, width - 0.5 - cx), max(cy - 0.5, height - 0.5 - cy) / 1.07
    f = math.hypot(ax, ay) / corner_theta_d
    return np.array([f, f * 1.07, cx, cy, coeffs[0], coeffs[1], coeffs[2], 0.0, 0.0, coeffs[3], 1.0, 0.0], dtype=np.float64)


def perspective_row12(width=52, height=36, coeffs=cref.TEST_COEFFS, scale=1.0):
    return np.concatenate([cref.camera_row(width, height, coeffs, scale), [0.0, 0.0, 0.0]])


def is_fisheye(row):
    return len(row) == 12 and float(row[10]) != 0.0


def _k(row):
    return float(row[4]), float(row[5]), float(row[6]), float(row[9])


def fisheye_forward(row, theta):
    k1, k2, k3, k4 = _k(row)
    t = np.asarray(theta, np.float64)
    return t * (1.0 + k1 * t ** 2 + k2 * t ** 4 + k3 * t ** 6 + k4 * t ** 8)


def fisheye_inverse(row, theta_d):
    """The smallest theta in [0, pi] with forward(theta) = theta_d, by bisection (forward must be increasing there) -> (theta, residual)."""
    td = np.asarray(theta_d, np.float64)
    lo, hi = np.zeros_like(td), np.full_like(td, math.pi)
    assert np.all(fisheye_forward(row, hi) >= td), "theta_d beyond the model's reach at theta = pi"
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        below = fisheye_forward(row, mid) < td
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    th = 0.5 * (lo + hi)
    return th, np.abs(fisheye_forward(row, th) - td)


def newton_theta(row, theta_d, iterations=10):
    """The kernel's solve, float64: exactly `iterations` steps from theta_d, a step with |f'| <= 1e-12 skipped, then clipped to [0, pi]."""
    k1, k2, k3, k4 = _k(row)
    td = np.asarray(theta_d, np.float64)
    th = td.copy()
    for _ in range(iterations):
        t2 = th * th
        f = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td
        df = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))))
        ok = np.abs(df) > 1e-12
        th = np.where(ok, th - f / np.where(ok, df, 1.0), th)
    return np.clip(th, 0.0, math.pi)


def _direction_from_theta(xd, yd, td, th):
    safe = np.where(td == 0.0, 1.0, td)
    s = np.sin(th) / safe
    v = np.stack([xd * s, -(yd * s), -np.cos(th)], axis=-1)
    v[td == 0.0] = (0.0, 0.0, -1.0)
    return v


def fisheye_camera_direction(row, py, px, solve=None):
    """Camera-space unit direction [...,3] of the image point (px, py) (pixel centre = index + .5), float64."""
    fx, fy, cx, cy = (float(v) for v in row[:4])
    xd, yd = (np.asarray(px, np.float64) - cx) / fx, (np.asarray(py, np.float64) - cy) / fy
    td = np.sqrt(xd * xd + yd * yd)
    if solve is None:
        th, res = fisheye_inverse(row, td)
        assert res.max() < 1e-14, res.max()
    else:
        th = solve(row, td)
    return _direction_from_theta(xd, yd, td, th)


def rays(c2w, row, y, x):
    """Literal definition, float64 -> origins [...,3], directions [...,3], pixel_area [...]; a perspective row: capture_reference.rays."""
    if not is_fisheye(row):
        return cref.rays(c2w, np.asarray(row, np.float64)[:9], y, x)
    c2w = np.asarray(c2w, np.float64)
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)

    def direction(yy, xx):
        w = np.einsum("ij,...j->...i", c2w[:3, :3], fisheye_camera_direction(row, yy + 0.5, xx + 0.5))
        return w / np.linalg.norm(w, axis=-1, keepdims=True)

    d = direction(y, x)
    area = np.linalg.norm(d - direction(y, x + 1.0), axis=-1) * np.linalg.norm(d - direction(y + 1.0, x), axis=-1)
    return np.broadcast_to(c2w[:3, 3], d.shape), d, area


def rays_f32(c2w, row32, y, x):
    """The kernel recipe step by step in the precision include/rsn.h gives each step -> directions float32 [...,3], pixel_area float32
    [...].  Sizes the GPU tests' bounds; never the expected value."""
    row32 = np.asarray(row32, np.float32)
    if not is_fisheye(row32):
        return cref.rays_f32(c2w, row32[:9], y, x)
    f = np.float32
    R = np.asarray(c2w, np.float32)
    row = row32.astype(np.float64)
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    v0 = fisheye_camera_direction(row, y + 0.5, x + 0.5, solve=newton_theta)
    vx = fisheye_camera_direction(row, y + 0.5, x + 1.5, solve=newton_theta)
    vy = fisheye_camera_direction(row, y + 1.5, x + 0.5, solve=newton_theta)
    v, e = v0.astype(f), [(vx - v0).astype(f), (vy - v0).astype(f)]
    w = [v[..., 0] * R[i, 0] + v[..., 1] * R[i, 1] + v[..., 2] * R[i, 2] for i in range(3)]
    a2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    a = np.sqrt(a2)
    nb = []
    for ee in e:
        g = [ee[..., 0] * R[i, 0] + ee[..., 1] * R[i, 1] + ee[..., 2] * R[i, 2] for i in range(3)]
        wg = w[0] * g[0] + w[1] * g[1] + w[2] * g[2]
        gg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
        db2 = f(2.0) * wg + gg
        b = np.sqrt(a2 + db2)
        s, t = (db2 / (a + b)) / (a * b), f(1.0) / b
        q = [w[i] * s - g[i] * t for i in range(3)]
        nb.append(np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]))
    d = np.stack([w[i] / a for i in range(3)], axis=-1)
    assert d.dtype == np.float32 and nb[0].dtype == np.float32
    return d, nb[0] * nb[1]


# ------------------------------------------------------------------------------------------------ masks and lists
def level_liveness(masks, level):
    """masks [N,H,W] (non-zero = live) -> bool [N, H >> l, W >> l]: a level pixel is live when all 2^l x 2^l pixels under it are."""
    s = 1 << level
    n, h, w = masks.shape
    assert h % s == 0 and w % s == 0
    return (np.asarray(masks) != 0).reshape(n, h // s, s, w // s, s).all(axis=(2, 4))


def live_lists(masks, levels):
    """-> [uint32 array per level]: the ascending flat level-pixel indices that are live."""
    return [np.flatnonzero(level_liveness(masks, l)).astype(np.uint32) for l in range(levels)]


def named_masks(N=5, H=36, W=52, seed=3):
    """The masks of the GPU tests, by name."""
    rng = np.random.default_rng(seed)
    out = {"all_live": np.ones((N, H, W), np.uint8)}
    out["dead_image"] = out["all_live"].copy()
    out["dead_image"][N // 2] = 0
    out["last_pixel"] = np.zeros((N, H, W), np.uint8)
    out["last_pixel"][-1, -1, -1] = 1
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out["checkerboard"] = np.broadcast_to(((yy + xx) % 2).astype(np.uint8), (N, H, W)).copy()
    out["rectangle"] = np.zeros((N, H, W), np.uint8)
    out["rectangle"][:, 5:H - 6, 3:W - 9] = 1  # edges that are no multiples of 4 (nor of 2, on three sides)
    out["random30"] = (rng.random((N, H, W)) < 0.3).astype(np.uint8)
    # 30 % of the pixels alone leave no level-2 pixel live (0.3^16): for the multi-level draws, 30 % of the 4 x 4 blocks are live as
    # well, so that every level has its own, different list
    blocks = (rng.random((N, H // 4, W // 4)) < 0.3).astype(np.uint8)
    out["random30_blocks"] = out["random30"] | np.kron(blocks, np.ones((4, 4), np.uint8))
    return out


def sample_through_lists(n_images, height, width, levels, lists, n_rays, seed, rank, step):
    """-> (level int64 [R], indices int64 [R,3]) of rsn_sample_capture_rays_live; lists=None: every pixel."""
    ctr = np.zeros((n_rays, 4), dtype=np.uint64)
    ctr[:, 0] = step
    ctr[:, 1] = np.arange(n_rays)
    rnd = philox4x32_10(ctr, (seed, rank)).astype(np.uint64)
    u, v = rnd[:, 0], rnd[:, 1]
    lvl = ((v * np.uint64(levels)) >> np.uint64(32)).astype(np.int64)
    hl, wl = height >> lvl, width >> lvl
    flat = np.empty(n_rays, np.int64)
    for l in range(levels):
        at = lvl == l
        if lists is None:
            flat[at] = ((u[at] * np.uint64(n_images * (height >> l) * (width >> l))) >> np.uint64(32)).astype(np.int64)
        else:
            pos = ((u[at] * np.uint64(len(lists[l]))) >> np.uint64(32)).astype(np.int64)
            flat[at] = lists[l][pos]
    hw = hl * wl
    rem = flat % hw
    return lvl, np.stack([flat // hw, rem // wl, rem % wl], axis=-1)


# ------------------------------------------------------------------------------------------------ scenes on disk
def fisheye_sphere_image(c2w, row, H, W, radius=0.8):
    """capture_reference.sphere_image through a fisheye row: float64 [H,W,3]."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    o, d, _ = rays(c2w, row, yy, xx)
    light = np.array([0.5, 0.8, 0.3]) / np.linalg.norm([0.5, 0.8, 0.3])
    b = (o * d).sum(-1)
    disc = b * b - ((o * o).sum(-1) - radius ** 2)
    t = -b - np.sqrt(np.clip(disc, 0, None))
    nrm = o + t[..., None] * d
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    shade = 0.25 + 0.75 * np.clip(nrm @ light, 0, None)
    return np.where((disc > 0)[..., None], shade[..., None] * np.array([0.85, 0.35, 0.25]), 1.0)


KEYS12 = ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "k3", "p1", "p2", "k4")


def write_lens_capture(root, images, c2w, rows, masks=None, mask_modes=None, image_dir="images", mask_dir="masks", declared_scale=1,
                       frame_extra=None):
    """A nerfstudio-format directory with per-frame cameras from 9- or 12-column rows (a fisheye row is written as OPENCV_FISHEYE
    with its k4).  images uint8 [N,H,W,3|4] are saved under image_dir while the JSON names images/ (so that image_dir = "images_2"
    with declared_scale = 2 writes what ns-process-data puts beside the full-size set: the JSON's intrinsics and w, h are the rows'
    times declared_scale).  masks: None or {frame index: uint8 [H,W]} (non-zero = live), saved under mask_dir in mask_modes[i]
    ("L", "RGB" or "RGBA"; default "L") while the JSON names masks/."""
    from PIL import Image

    os.makedirs(os.path.join(root, image_dir), exist_ok=True)
    N, H, W = images.shape[:3]
    frames = []
    for i in range(N):
        name = f"frame_{i:05d}.png"
        Image.fromarray(images[i]).save(os.path.join(root, image_dir, name))
        row = np.asarray(rows[i], np.float64)
        row = np.concatenate([row, [0.0, 0.0, 0.0]]) if len(row) == 9 else row
        fr = {"file_path": "images/" + name, "transform_matrix": np.vstack([np.asarray(c2w[i], np.float64)[:3, :4], [[0, 0, 0, 1]]]).tolist(),
              "camera_model": "OPENCV_FISHEYE" if row[10] != 0.0 else "OPENCV", "w": W * declared_scale, "h": H * declared_scale}
        fr.update({k: float(v) * (declared_scale if j < 4 else 1) for j, (k, v) in enumerate(zip(KEYS12, row))})
        if row[10] == 0.0:
            del fr["k4"]
        if masks is not None and i in masks:
            os.makedirs(os.path.join(root, mask_dir), exist_ok=True)
            mode = (mask_modes or {}).get(i, "L")
            m8 = (np.asarray(masks[i]) != 0).astype(np.uint8) * 255
            if mode == "L":
                im = Image.fromarray(m8, "L")
            else:  # the first channel carries the mask; the others say the opposite, so that a reader of another channel is found out
                chans = [m8] + [255 - m8] * (len(mode) - 1)
                im = Image.fromarray(np.stack(chans, axis=-1), mode)
            im.save(os.path.join(root, mask_dir, name))
            fr["mask_path"] = "masks/" + name
        fr.update((frame_extra or {}).get(i, {}))
        frames.append(fr)
    with open(os.path.join(root, "transforms.json"), "w") as fh:
        json.dump({"frames": frames}, fh)
    return root
