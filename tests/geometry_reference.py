"""Host restatement (numpy, float64) of the geometry metrics of include/rsn.h ("geometry metrics": rsn_normal_error), the literal
multinerf formula it stands for, the seeded inputs the kernel tests share, and the sphere toy with analytic normal maps."""
import math

import numpy as np

from tests.data_reference import camera_rays

ALPHAS = (0, 1, 51, 128, 255)
PLANTED_GT = (200, 90, 30)  # bytes of the planted rows' ground truth: 2u - 255 = (145, -75, -195)


def decode(gt_normals):
    """uint8 [...,3] -> float64 [...,3]: 2u - 255, the exact integers the kernel compares against (255 times the encoded normal)."""
    return 2.0 * np.asarray(gt_normals).astype(np.float64) - 255.0


def valid_mask(gt_normals, alpha):
    """alpha > 0 and some |2u - 255| > 1: the bytes 127 / 128 in all three channels are the background of a normal map."""
    return (np.asarray(alpha).astype(np.int64) > 0) & (np.abs(decode(gt_normals)).max(axis=-1) > 1.0)


def angle_deg(p, g):
    """atan2(|p x g|, p . g) in degrees, float64 [...]; 90 where both vanish (a zero prediction)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    c = np.cross(p, g)
    s = np.sqrt((c * c).sum(-1))
    d = (p * g).sum(-1)
    theta = np.where((s == 0.0) & (d == 0.0), math.pi / 2.0, np.arctan2(s, d))
    return theta * (180.0 / math.pi)


def multinerf_angle_deg(p, g, eps=1e-20):
    """The literal multinerf compute_normal_mae angle: arccos(clip(<l2-normalised p, l2-normalised g>, -1, 1)) in degrees, float64."""
    def l2n(x):
        x = np.asarray(x, dtype=np.float64)
        return x / np.sqrt(np.maximum((x * x).sum(-1, keepdims=True), eps))

    return np.degrees(np.arccos(np.clip((l2n(p) * l2n(g)).sum(-1), -1.0, 1.0)))


def reduce(error_map, valid, alpha, accumulation):
    """The four outputs from a per-pixel error map, in float64: (S1/S2, S2/255, S3/P, n); the first is NaN when nothing is valid."""
    a = np.asarray(alpha).astype(np.float64).reshape(-1)
    v = np.asarray(valid).reshape(-1)
    e = np.asarray(error_map, dtype=np.float64).reshape(-1)
    s1, s2 = float((a[v] * e[v]).sum()), float(a[v].sum())
    s3 = 0.0 if accumulation is None else float(np.abs(np.asarray(accumulation, dtype=np.float64).reshape(-1) - a / 255.0).sum())
    return np.array([s1 / s2 if s2 > 0.0 else math.nan, s2 / 255.0, s3 / a.size, float(v.sum())])


def normal_error(normals, accumulation, gt_normals, gt_rgba, rotation=None):
    """-> {"error_map" float64 [P] (0 where invalid), "valid" bool [P], "out" float64 [4]}; inputs [P,3], [P] or None, uint8 [P,3],
    uint8 [P,4]; rotation [3,3] (its given values, taken to float64): the decoded ground truth is rotated by it first."""
    g = decode(gt_normals).reshape(-1, 3)
    alpha = np.asarray(gt_rgba).reshape(-1, 4)[:, 3]
    valid = valid_mask(np.asarray(gt_normals).reshape(-1, 3), alpha)
    if rotation is not None:
        g = g @ np.asarray(rotation, dtype=np.float64).reshape(3, 3).T
    emap = np.where(valid, angle_deg(np.asarray(normals, dtype=np.float64).reshape(-1, 3), g), 0.0)
    return {"error_map": emap, "valid": valid, "out": reduce(emap, valid, alpha, accumulation)}


def kernel_inputs(n_pixels, seed=0, all_alpha_zero=False):
    """Seeded inputs of the kernel tests for P = n_pixels: predicted rows with norms from 1e-2 to 1.5 (log-uniform) in random
    directions, random ground-truth bytes, alphas from ALPHAS, accumulations in [0, 1]; then planted, as far as P reaches, row 0
    exactly parallel to its ground truth (p = g / 256, exact in float32), row 1 exactly antiparallel, row 2 a zero prediction, row 3 an
    invalid ground truth (127, 128, 128) under alpha 255, row 4 alpha 0 over a good normal; for P > 5 the LAST row is valid with alpha
    255, so that the pixel of a lane's second trip counts.  -> normals float32 [P,3], accumulation float32 [P], gt_normals uint8 [P,3],
    gt_rgba uint8 [P,4]."""
    P = int(n_pixels)
    rng = np.random.default_rng([seed, P])
    d = rng.standard_normal((P, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    norms = np.exp(rng.uniform(math.log(1e-2), math.log(1.5), size=(P, 1)))
    normals = (d * norms).astype(np.float32)
    gt = rng.integers(0, 256, size=(P, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, size=(P, 4), dtype=np.uint8)
    rgba[:, 3] = rng.choice(np.array(ALPHAS, dtype=np.uint8), size=P)
    acc = rng.uniform(0.0, 1.0, size=P).astype(np.float32)
    g = (2.0 * np.array(PLANTED_GT) - 255.0).astype(np.float32)
    planted = [(g / 256.0, PLANTED_GT, 255), (-g / 256.0, PLANTED_GT, 255), (np.zeros(3, np.float32), PLANTED_GT, 255),
               (normals[min(3, P - 1)], (127, 128, 128), 255), (normals[min(4, P - 1)], PLANTED_GT, 0)]
    for i, (p, u, a) in enumerate(planted[:P]):
        normals[i], gt[i], rgba[i, 3] = p, u, a
    if P > 5:
        gt[P - 1], rgba[P - 1, 3] = (30, 200, 90), 255
    if all_alpha_zero:
        rgba[:, 3] = 0
    return normals, acc, gt, rgba


def rotation_matrix(ax=0.3, ay=-1.1, az=2.0):
    """A non-trivial orthonormal matrix, float32 [3,3] (Rz Ry Rx of the three angles, rounded to float32)."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (rz @ ry @ rx).astype(np.float32)


def _look_at(pos):
    back = pos / np.linalg.norm(pos)
    right = np.cross(np.array([0.0, 0.0, 1.0]), back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.concatenate([np.stack([right, up, back], 1), pos[:, None]], 1).astype(np.float32)


def sphere_views(n, H=48, W=48, offset=0.0):
    """The Lambert sphere of tests/test_data_gpu._sphere_scene (radius 0.8 at the origin, white background, seen from a radius-4
    shell) with its analytic world-space normals: -> (images float64 [n,H,W,3], poses float32 [n,3,4], focal, normals float64
    [n,H,W,3]: the unit outward normal where the pixel's ray hits the sphere, zero -- which encodes as the bytes 128 -- elsewhere)."""
    k = np.arange(n) + 0.5 + offset
    z = np.clip(0.8 * (1 - 2 * k / (n + 1)), -0.8, 0.8)
    phi = k * math.pi * (3 - math.sqrt(5))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1)
    poses = np.stack([_look_at(4.0 * d) for d in dirs])
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    light = np.array([0.5, 0.8, 0.3]) / np.linalg.norm([0.5, 0.8, 0.3])
    base = np.array([0.85, 0.35, 0.25])
    ims, nms = [], []
    for p in poses:
        o, d, _ = camera_rays(p.astype(np.float64), focal, focal, W / 2, H / 2, yy, xx)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - 0.8 ** 2)
        t = -b - np.sqrt(np.clip(disc, 0, None))
        nrm = o + t[..., None] * d
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        hit = (disc > 0)[..., None]
        shade = 0.25 + 0.75 * np.clip(nrm @ light, 0, None)
        ims.append(np.where(hit, shade[..., None] * base, 1.0))
        nms.append(np.where(hit, nrm, 0.0))
    return np.stack(ims), poses, focal, np.stack(nms)
