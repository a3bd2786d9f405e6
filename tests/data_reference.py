"""Host restatements (numpy) of the data-path recipes in include/rsn.h: Philox4x32-10 pixel sampling, nerfstudio 0.3's
perspective ray generation (float64, literal form), the white blend, and torchmetrics' SSIM (float64)."""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: (k0, k1) -> uint32 [..., 4] (Random123 philox4x32, 10 rounds)."""
    c = [np.asarray(ctr, dtype=np.uint64)[..., j].copy() for j in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r > 0:
            k0 = (k0 + np.uint64(_W0)) & _MASK
            k1 = (k1 + np.uint64(_W1)) & _MASK
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, axis=-1).astype(np.uint32)


def sample_indices(n_images, height, width, n_rays, seed, rank, step):
    """-> int64 [R, 3] (image, y, x) of rsn_sample_camera_rays."""
    ctr = np.zeros((n_rays, 4), dtype=np.uint64)
    ctr[:, 0] = step
    ctr[:, 1] = np.arange(n_rays)
    u = philox4x32_10(ctr, (seed, rank))[:, 0].astype(np.uint64)
    flat = (u * np.uint64(n_images * height * width)) >> np.uint64(32)
    flat = flat.astype(np.int64)
    hw = height * width
    i = flat // hw
    rem = flat % hw
    return np.stack([i, rem // width, rem % width], axis=-1)


def camera_rays(c2w, fx, fy, cx, cy, y, x):
    """nerfstudio 0.3 _generate_rays_from_coords (perspective) in float64, literal form.  c2w [..., 3, 4] broadcast
    against y, x [...] -> origins [..., 3], directions [..., 3], pixel_area [...]."""
    c2w = np.asarray(c2w, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)

    def direction(xx, yy):
        v = np.stack([(xx + 0.5 - cx) / fx, -(yy + 0.5 - cy) / fy, -np.ones_like(xx)], axis=-1)
        w = np.einsum("...ij,...j->...i", c2w[..., :3, :3], v)
        return w / np.linalg.norm(w, axis=-1, keepdims=True)

    d = direction(x, y)
    dx = np.linalg.norm(d - direction(x + 1.0, y), axis=-1)
    dy = np.linalg.norm(d - direction(x, y + 1.0), axis=-1)
    o = np.broadcast_to(c2w[..., :3, 3], d.shape)
    return o, d, dx * dy


def blend_white_f32(texels):
    """uint8 [..., 4] -> float32 [..., 3]: c/255 * a/255 + (1 - a/255), every operation in float32."""
    f = texels.astype(np.float32) / np.float32(255.0)
    return f[..., :3] * f[..., 3:4] + (np.float32(1.0) - f[..., 3:4])


def gaussian_taps(k=11, sigma=1.5):
    t = np.arange(k, dtype=np.float64) - (k - 1) / 2
    g = np.exp(-(t / sigma) ** 2 / 2)
    return g / g.sum()


def ssim(pred, target):
    """torchmetrics structural_similarity_index_measure (gaussian 11, sigma 1.5, k1 0.01, k2 0.03, data range from the
    images) of two [H, W, 3] images, in float64, over the full-window positions."""
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    H, W = p.shape[:2]
    L = max(p.max() - p.min(), t.max() - t.min())
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    g = gaussian_taps()

    def filt(a):
        h = sum(g[k] * a[:, k:k + W - 10] for k in range(11))
        return sum(g[k] * h[k:k + H - 10] for k in range(11))

    mp, mt = filt(p), filt(t)
    spp = filt(p * p) - mp * mp
    stt = filt(t * t) - mt * mt
    spt = filt(p * t) - mp * mt
    s = ((2 * mp * mt + c1) * (2 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2))
    return float(s.mean())
