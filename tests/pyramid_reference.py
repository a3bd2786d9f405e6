"""Host restatements (numpy) of the image-pyramid recipes in include/rsn.h: the levels as integer box sums of the white blend with
one float32 division, their layout in the one allocation, and the level + pixel draw of rsn_sample_pyramid_rays on top of
tests/data_reference.philox4x32_10."""
import numpy as np

from tests.data_reference import philox4x32_10


def pyramid_level(images, level):
    """images uint8 [N,H,W,4], level l >= 1 -> float32 [N, H >> l, W >> l, 3]: S = sum over the 2^l x 2^l box of
    c8 * a8 + 255 * (255 - a8) in integers, value = float32(S) / float32(65025 * 4^l)."""
    s = 1 << level
    n, h, w, _ = images.shape
    assert level >= 1 and h % s == 0 and w % s == 0
    im = images.astype(np.int64)
    term = im[..., :3] * im[..., 3:4] + 255 * (255 - im[..., 3:4])
    S = term.reshape(n, h // s, s, w // s, s, 3).sum(axis=(2, 4))
    assert S.max() < 2 ** 24 and 65025 * s * s < 2 ** 24  # both operands exact in float32
    return S.astype(np.float32) / np.float32(65025 * s * s)


def pyramid_level_float64(images, level):
    """The float64 box average of the float64 white blend c/255 * a/255 + (1 - a/255) (the definition the recipe rounds once)."""
    s = 1 << level
    n, h, w, _ = images.shape
    f = images.astype(np.float64) / 255.0
    blend = f[..., :3] * f[..., 3:4] + (1.0 - f[..., 3:4])
    return blend.reshape(n, h // s, s, w // s, s, 3).mean(axis=(2, 4))


def pyramid_offsets(n, h, w, levels):
    """offsets[l] = first pixel of level l >= 1 in the allocation, offsets[levels] = its size; offsets[0] unused."""
    off = [0, 0]
    for l in range(1, levels):
        off.append(off[-1] + n * (h >> l) * (w >> l))
    return off[:levels + 1]


def pyramid_flat(images, levels):
    """The whole allocation: float32 [offsets[levels], 3], level after level, image after image, row-major."""
    parts = [pyramid_level(images, l).reshape(-1, 3) for l in range(1, levels)]
    return np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)


def sample_levels_and_indices(n_images, height, width, levels, n_rays, seed, rank, step):
    """-> (level int64 [R], indices int64 [R,3] = (image, y, x) in the level's pixel coordinates) of rsn_sample_pyramid_rays."""
    ctr = np.zeros((n_rays, 4), dtype=np.uint64)
    ctr[:, 0] = step
    ctr[:, 1] = np.arange(n_rays)
    rnd = philox4x32_10(ctr, (seed, rank)).astype(np.uint64)
    u, v = rnd[:, 0], rnd[:, 1]
    lvl = ((v * np.uint64(levels)) >> np.uint64(32)).astype(np.int64)
    hl, wl = height >> lvl, width >> lvl
    total = (n_images * hl * wl).astype(np.uint64)
    assert int(total.max()) < 2 ** 32
    flat = ((u * total) >> np.uint64(32)).astype(np.int64)
    hw = hl * wl
    rem = flat % hw
    return lvl, np.stack([flat // hw, rem // wl, rem % wl], axis=-1)
