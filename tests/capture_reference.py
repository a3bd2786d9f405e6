"""Host restatements (numpy) of the capture recipes in include/rsn.h ("captures") and of the nerfstudio-format loader's rules, written
from those recipes and not from the kernels or the loader:

    distort / undistort      the OpenCV / COLMAP model in float64, and its inverse iterated to a residual below 1e-15
    rays                     origins, directions and pixel_area of a camera-table row by the literal definition, in float64
    rays_f32                 the kernel recipe with its float32 steps in float32; used ONLY to size the bounds of the GPU tests
    project                  a world direction pushed forward through the float64 model to pixel coordinates
    orient_and_center / split_indices
                             the pose normalisation and the fraction split as the loader's documentation words them
    sphere_image / write_capture
                             the Lambert sphere of tests/test_data_gpu.py rendered through a distorted camera, and a capture on disk
"""
import json
import math
import os

import numpy as np

# about 60 degrees of horizontal field of view on a 53-pixel-wide image, fx != fy, principal point off the centre
TEST_COEFFS = (-0.12, 0.03, -0.004, 0.002, -0.0015)  # k1 k2 k3 p1 p2


def camera_row(width=53, height=37, coeffs=TEST_COEFFS, scale=1.0):
    fx = 0.5 * width / math.tan(math.radians(30.0))
    return np.array([fx * scale, fx * 1.07 * scale, width / 2.0 - 0.7, height / 2.0 + 0.4, *coeffs], dtype=np.float64)


def distort(row, X, Y):
    k1, k2, k3, p1, p2 = (float(v) for v in row[4:9])
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    r2 = X * X + Y * Y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return X * rad + 2.0 * p1 * X * Y + p2 * (r2 + 2.0 * X * X), Y * rad + p1 * (r2 + 2.0 * Y * Y) + 2.0 * p2 * X * Y


def _jacobian(row, X, Y):
    k1, k2, k3, p1, p2 = (float(v) for v in row[4:9])
    r2 = X * X + Y * Y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + 2.0 * k2 * r2 + 3.0 * k3 * r2 * r2
    return (rad + 2.0 * X * X * drad + 2.0 * p1 * Y + 6.0 * p2 * X, 2.0 * X * Y * drad + 2.0 * p1 * X + 2.0 * p2 * Y,
            rad + 2.0 * Y * Y * drad + 6.0 * p1 * Y + 2.0 * p2 * X)


def undistort(row, Xd, Yd, iterations=None, tol=1e-15, max_iterations=100):
    """-> (X, Y, residual).  iterations=None: Newton until every point's residual is below tol (the reference); iterations=n: exactly
    n steps with the kernel's rule that a step whose |det J| <= 1e-12 leaves the point where it is."""
    Xd, Yd = np.asarray(Xd, np.float64), np.asarray(Yd, np.float64)
    X, Y = Xd.copy(), Yd.copy()
    res = np.full(Xd.shape, np.inf)
    for it in range(max_iterations if iterations is None else iterations):
        bx, by = distort(row, X, Y)
        rx, ry = bx - Xd, by - Yd
        res = np.maximum(np.abs(rx), np.abs(ry))
        if iterations is None and res.max() < tol:
            break
        j11, j12, j22 = _jacobian(row, X, Y)
        det = j11 * j22 - j12 * j12
        ok = np.abs(det) > 1e-12
        det = np.where(ok, det, 1.0)
        X = np.where(ok, X - (j22 * rx - j12 * ry) / det, X)
        Y = np.where(ok, Y - (j11 * ry - j12 * rx) / det, Y)
    bx, by = distort(row, X, Y)
    return X, Y, np.maximum(np.abs(bx - Xd), np.abs(by - Yd))


def _has_distortion(row):
    return bool(np.any(np.asarray(row)[4:9] != 0.0))


def camera_point(row, y, x):
    """The undistorted normalised point of the centre of pixel (y, x), float64."""
    fx, fy, cx, cy = (float(v) for v in row[:4])
    Xd, Yd = (np.asarray(x, np.float64) + 0.5 - cx) / fx, (np.asarray(y, np.float64) + 0.5 - cy) / fy
    if not _has_distortion(row):
        return Xd, Yd
    X, Y, res = undistort(row, Xd, Yd)
    assert res.max() < 1e-15, res.max()
    return X, Y


def rays(c2w, row, y, x):
    """Literal definition, float64: -> origins [...,3], directions [...,3], pixel_area [...]."""
    c2w = np.asarray(c2w, np.float64)

    def direction(yy, xx):
        X, Y = camera_point(row, yy, xx)
        w = np.einsum("ij,...j->...i", c2w[:3, :3], np.stack([X, -Y, -np.ones_like(X)], axis=-1))
        return w / np.linalg.norm(w, axis=-1, keepdims=True)

    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    d = direction(y, x)
    area = np.linalg.norm(d - direction(y, x + 1.0), axis=-1) * np.linalg.norm(d - direction(y + 1.0, x), axis=-1)
    return np.broadcast_to(c2w[:3, 3], d.shape), d, area


def rays_f32(c2w, row32, y, x):
    """The kernel recipe, step by step in the precision include/rsn.h gives each step (row32: the float32 row the device holds):
    -> directions float32 [...,3], pixel_area float32 [...].  Sizes the GPU tests' bounds; never the expected value."""
    f = np.float32
    row32 = np.asarray(row32, np.float32)
    R = np.asarray(c2w, np.float32)
    y, x = np.asarray(y), np.asarray(x)
    if _has_distortion(row32):
        row = row32.astype(np.float64)
        fx, fy, cx, cy = row[:4]

        def solve(yy, xx):
            return undistort(row, (xx - cx) / fx, (yy - cy) / fy, iterations=10)[:2]

        X0, Y0 = solve(y + 0.5, x + 0.5)
        Xx, Yx = solve(y + 0.5, x + 1.5)
        Xy, Yy = solve(y + 1.5, x + 0.5)
        vx, vy = X0.astype(f), (-Y0).astype(f)
        e = [((Xx - X0).astype(f), (-(Yx - Y0)).astype(f)), ((Xy - X0).astype(f), (-(Yy - Y0)).astype(f))]
    else:
        fx, fy, cx, cy = row32[:4]
        vx = (x.astype(f) + f(0.5) - cx) / fx
        vy = -((y.astype(f) + f(0.5) - cy) / fy)
        zero = np.zeros_like(vx)
        e = [(zero + f(1.0) / fx, zero), (zero, zero - f(1.0) / fy)]
    w = [vx * R[i, 0] + vy * R[i, 1] + f(-1.0) * R[i, 2] for i in range(3)]
    a2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    a = np.sqrt(a2)
    nb = []
    for ex, ey in e:
        g = [ex * R[i, 0] + ey * R[i, 1] for i in range(3)]
        wg = w[0] * g[0] + w[1] * g[1] + w[2] * g[2]
        gg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2]
        db2 = f(2.0) * wg + gg
        b = np.sqrt(a2 + db2)
        s, t = (db2 / (a + b)) / (a * b), f(1.0) / b
        ee = [w[i] * s - g[i] * t for i in range(3)]
        nb.append(np.sqrt(ee[0] * ee[0] + ee[1] * ee[1] + ee[2] * ee[2]))
    d = np.stack([w[i] / a for i in range(3)], axis=-1)
    assert d.dtype == np.float32 and nb[0].dtype == np.float32
    return d, nb[0] * nb[1]


def project(c2w, row, d):
    """World directions [...,3] -> pixel coordinates (u, v) through the float64 model (a pixel centre is at x + .5, y + .5)."""
    c2w, d = np.asarray(c2w, np.float64), np.asarray(d, np.float64)
    v = np.einsum("ji,...j->...i", c2w[:3, :3], d)
    X, Y = v[..., 0] / -v[..., 2], v[..., 1] / v[..., 2]
    Xd, Yd = distort(row, X, Y)
    return float(row[0]) * Xd + float(row[2]), float(row[1]) * Yd + float(row[3])


# ------------------------------------------------------------------------------------------------ loader rules
def orient_and_center(c2w, orientation="up", center="poses"):
    """-> (poses [N,3,4], transform [3,4]).  "poses": subtract the mean camera position; "up": rotate the normalised mean of the
    cameras' up axes onto +z about the axis up x z by the angle between them (antiparallel: a turn of pi about x)."""
    P = np.asarray(c2w, np.float64)[:, :3, :4]
    t = P[:, :, 3].mean(0) if center == "poses" else np.zeros(3)
    R = np.eye(3)
    if orientation == "up":
        up = P[:, :, 1].mean(0)
        up /= np.linalg.norm(up)
        axis = np.cross(up, [0.0, 0.0, 1.0])
        s, c = np.linalg.norm(axis), up[2]
        if c < -1.0 + 1e-8:
            R = np.diag([1.0, -1.0, -1.0])
        elif s > 0.0:
            k = axis / s
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            R = c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k)
    out = np.empty_like(P)
    for i in range(len(P)):
        out[i, :, :3] = R @ P[i, :, :3]
        out[i, :, 3] = R @ (P[i, :, 3] - t)
    return out, np.concatenate([R, (-R @ t)[:, None]], axis=1)


def split_indices(n, fraction=0.9):
    """-> (i_train, i_eval): num_train = ceil(n * fraction), i_train = linspace(0, n - 1, num_train) truncated, eval the complement."""
    num_train = math.ceil(n * fraction)
    i_train = [int(v) for v in np.linspace(0, n - 1, num_train)]
    return np.array(i_train), np.array([i for i in range(n) if i not in set(i_train)], dtype=int)


# ------------------------------------------------------------------------------------------------ scenes on disk
def look_at(pos):
    back = pos / np.linalg.norm(pos)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], 1), pos[:, None]], 1)


def shell_poses(n, radius=4.0, offset=0.0):
    """The camera shell of tests/test_data_gpu._sphere_scene."""
    k = np.arange(n) + 0.5 + offset
    z = np.clip(0.8 * (1 - 2 * k / (n + 1)), -0.8, 0.8)
    phi = k * math.pi * (3 - math.sqrt(5))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1)
    return np.stack([look_at(radius * d) for d in dirs])


def sphere_image(c2w, row, H, W, radius=0.8):
    """The Lambert sphere of tests/test_data_gpu._sphere_scene (white background) through the camera `row`: float64 [H,W,3]."""
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


def write_capture(root, images, c2w, rows, names=None, per_frame=True, extra=None, frame_extra=None, quality=95):
    """A nerfstudio-format directory: images uint8 [N,H,W,3|4] saved under images/ by their names' extensions (.png / .jpg), the
    cameras per frame or (per_frame=False: row 0) globally.  extra / frame_extra[i]: further top-level / per-frame entries."""
    from PIL import Image

    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    N, H, W = images.shape[:3]
    names = names or [f"images/frame_{i:05d}.png" for i in range(N)]
    keys = ("fl_x", "fl_y", "cx", "cy", "k1", "k2", "k3", "p1", "p2")
    meta = {"camera_model": "OPENCV"}
    if not per_frame:
        meta.update({k: float(v) for k, v in zip(keys, rows[0])}, w=W, h=H)
    frames = []
    for i in range(N):
        im = Image.fromarray(images[i])
        if names[i].lower().endswith((".jpg", ".jpeg")):
            im.convert("RGB").save(os.path.join(root, names[i]), quality=quality)
        else:
            im.save(os.path.join(root, names[i]))
        fr = {"file_path": names[i], "transform_matrix": np.vstack([np.asarray(c2w[i], np.float64)[:3, :4], [[0, 0, 0, 1]]]).tolist()}
        if per_frame:
            fr.update({k: float(v) for k, v in zip(keys, rows[i])}, w=W, h=H)
        fr.update((frame_extra or {}).get(i, {}))
        frames.append(fr)
    meta["frames"] = frames
    meta.update(extra or {})
    with open(os.path.join(root, "transforms.json"), "w") as fh:
        json.dump(meta, fh)
    return root
