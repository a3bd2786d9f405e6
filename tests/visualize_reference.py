"""numpy restatement, in fp64, of the rsn_visualize contract of include/rsn.h, and the shared cases of its CPU and GPU tests.

expected(kind, x, alpha, lo, hi, lut) -> (code, ambiguous, alt, joint):
  code       uint8 [N,3]: the byte the contract gives when every step is carried out exactly on the fp32 inputs;
  ambiguous  bool [N,3]: a value that is about to be truncated lies within AMBIGUITY of an integer, so that the device, whose
             steps are rounded to fp32, may land on the other side of it;
  alt        uint8 [N,3]: the byte on that other side (equal to code where nothing is ambiguous).
  joint      bool [N]: the pixel's ambiguity is its table index (RSN_VIS_LUT), which its three channels share: the device
             pixel is code in all three channels or alt in all three.
A device byte must EQUAL code outside the ambiguous set, and be code or alt inside it (check()).

Two truncations exist: q(v) = (int)(v*255 + 0.5), and the table index k = (int)(t*255) of RSN_VIS_LUT.
  * q: v*255 + 0.5 within AMBIGUITY of an integer m: the other byte is m - 1 or m, whichever code is not.
  * k: t*255 within AMBIGUITY of an integer m (not at the ends 0 and 255 of the table): the other entry is m - 1 or m; alt is
    the byte of that entry.  A pixel ambiguous in both ways at once would need more than two admissible bytes; expected()
    refuses such an input (AssertionError) rather than widen the rule, and the cases below contain none.
AMBIGUITY = 1e-4: every quantity is at most 255.5 and passes through at most six correctly rounded fp32 operations, so the
device value lies within about 6 * 255.5 * 2^-24 = 9e-5 of the fp64 one.

A saturated t is exact on both sides -- sat() returns the constants 0 and 1 -- whenever the unsaturated value is not itself
within rounding of the bound it is clamped to: for u = (x - lo)/(hi - lo) beyond [0, 1] by more than SAT_MARGIN, for x == lo and
x == hi (0 / d and d / d), for NaN and the infinities, t*255 is exactly 0 or 255 and is not flagged."""
import numpy as np

RGB, UNIT, GRAY, LUT = 0, 1, 2, 3
KINDS = {"rgb": RGB, "unit": UNIT, "gray": GRAY, "lut": LUT}
AMBIGUITY = 1e-4
SAT_MARGIN = 1e-6  # many fp32 roundings of a value near 1
MAX_AMBIGUOUS_SHARE = 0.01


def sat(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0.0, np.where(v > 1.0, 1.0, v), 0.0)  # NaN compares false: 0


def _near_integer(v):
    return np.abs(v - np.rint(v)) < AMBIGUITY


def _q(v):
    """v [..] in [0, 1] -> (code, ambiguous, alt)."""
    s = v * 255.0 + 0.5
    code = np.floor(s).astype(np.int64)
    amb = _near_integer(s)
    m = np.rint(s).astype(np.int64)
    alt = np.where(amb, np.where(code == m, m - 1, m), code)
    return code, amb, np.clip(alt, 0, 255)


def expected(kind, x, alpha=None, lo=0.0, hi=1.0, lut=None):
    """x: fp32 [N,3] (RGB, UNIT) or [N] (GRAY, LUT); alpha fp32 [N] or None; lut fp32 [256,3]."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    a = np.ones(n) if alpha is None else sat(np.asarray(alpha, dtype=np.float32).reshape(n))
    a = a[:, None]
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    over = lambda c: c * a + (1.0 - a)  # noqa: E731
    joint = np.zeros(n, dtype=bool)
    if kind in (RGB, UNIT):
        c = sat(x.reshape(n, 3) * 0.5 + 0.5 if kind == UNIT else x.reshape(n, 3))
        code, amb, alt = _q(over(c))
    else:
        x = x.reshape(n)
        with np.errstate(invalid="ignore", over="ignore"):
            u = (x - lo) / (hi - lo)
        t = sat(u)
        if kind == GRAY:
            code, amb, alt = _q(over(np.repeat(t[:, None], 3, axis=1)))
        else:
            table = np.asarray(lut, dtype=np.float32).astype(np.float64)
            s = t * 255.0
            k = np.floor(s).astype(np.int64)
            with np.errstate(invalid="ignore"):
                exact_end = np.isnan(u) | (u <= -SAT_MARGIN) | (u >= 1.0 + SAT_MARGIN) | (x == lo) | (x == hi)
            k_amb = _near_integer(s) & ~exact_end
            m = np.rint(s).astype(np.int64)
            k_alt = np.clip(np.where(k_amb, np.where(k == m, m - 1, m), k), 0, 255)
            code, amb_q, alt_q = _q(over(table[k]))
            code_other, amb_other, _ = _q(over(table[k_alt]))
            both = k_amb[:, None] & (amb_q | amb_other)
            assert not both.any(), "a pixel is ambiguous in its table index and in its quantisation at once: choose another input"
            amb = amb_q | k_amb[:, None]
            alt = np.where(k_amb[:, None], code_other, alt_q)
            joint = k_amb
    return code.astype(np.uint8), amb, alt.astype(np.uint8), joint


def ambiguous_pixels(amb):
    return int(np.count_nonzero(amb.any(axis=1)))


def check(got, code, amb, alt, joint):
    """got uint8 [N,3] from the device against expected(): -> error string or None."""
    got = np.asarray(got).reshape(code.shape)
    bad = (got != code) & ~(amb & (got == alt))
    bad |= (joint & ~((got == code).all(axis=1) | (got == alt).all(axis=1)))[:, None]
    if bad.any():
        i = np.argwhere(bad)[0]
        return (f"{int(bad.sum())} bytes differ; first at pixel {i[0]} channel {i[1]}: device {got[tuple(i)]}, expected "
                f"{code[tuple(i)]}" + (f" or {alt[tuple(i)]}" if amb[tuple(i)] else ""))
    return None


# ------------------------------------------------------------------------------------------------ shared cases
SHAPES = ((1, 1), (3, 5), (7, 67))  # 7 x 67 = 469 pixels: more than one 256-lane workgroup, the last partial, no multiple of 64
TILES = ("tight", "inset")          # pitch = width, x0 = 0  /  pitch = width + 5, x0 = 2
RANGE = (0.0, 1.0)                  # lo / hi of the randomised GRAY and LUT cases
SPECIAL_RANGE = (2.0, 6.0)          # of the special-value cases: the model's collider planes


def tile_geometry(width, tile):
    return (width, 0) if tile == "tight" else (width + 5, 2)


def ramp_lut():
    return np.repeat((np.arange(256, dtype=np.float32) / np.float32(255.0))[:, None], 3, axis=1)


SEED = 0  # with it no case of fewer than 100 pixels holds an ambiguous one (one such pixel would be over the 1 % cap by itself)


def random_case(kind, height, width, with_alpha):
    """Inputs of one randomised case: uniform on [-0.25, 1.25], one seed per (kind, shape, alpha)."""
    rng = np.random.default_rng([SEED, kind, height, width, int(with_alpha)])
    n = height * width
    x = rng.uniform(-0.25, 1.25, size=(n, 3) if kind in (RGB, UNIT) else (n,)).astype(np.float32)
    if kind == UNIT:
        x = (x * 2.0 - 1.0).astype(np.float32)  # a unit vector's components, with the same overshoot
    alpha = rng.uniform(-0.25, 1.25, size=n).astype(np.float32) if with_alpha else None
    return x, alpha


def special_values(kind):
    """-> (x, alpha): every special x against every special alpha.  For GRAY and LUT, SPECIAL_RANGE is the range."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    ks = np.float32([1, 37, 128, 254]) / np.float32(255.0)
    base = [nan, inf, -inf, np.float32(-0.0), -1.0, 2.0, 0.0, 1.0, *ks]
    if kind in (GRAY, LUT):
        lo, hi = SPECIAL_RANGE
        base += [lo, hi, lo - 0.5, hi + 0.5, -1e30, 1e30, 3.1, 4.6, 5.5]
    xs = np.float32(base)
    als = np.float32([nan, inf, -inf, np.float32(-0.0), -1.0, 2.0, 0.0, 1.0, *ks])
    x = np.repeat(xs, len(als))
    alpha = np.tile(als, len(xs))
    if kind in (RGB, UNIT):
        x = np.stack([x, np.roll(x, len(als)), np.roll(x, 3 * len(als))], axis=1)  # three different specials per pixel
        if kind == UNIT:
            with np.errstate(invalid="ignore"):
                x = (x * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    return np.ascontiguousarray(x, dtype=np.float32), alpha
