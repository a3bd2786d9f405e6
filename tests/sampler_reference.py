"""fp64 references, inputs and the comparison rule for the two sampling kernels, rsn_sample_spaced and rsn_sample_pdf
(csrc/rsn_render.hip).  The reference is oracle/cpu_ref.py (spaced_bins / pdf_bins) under default_dtype(float64) on the float32
input bits; the same functions in float32 are the oracle whose own error sets every bound (field_maths_reference.compare: factor 4
over the oracle's worst error of the class, plus its floor).  Nothing here is measured on a kernel.

For the PDF sampler the reference also restates the inverse CDF in fp64 (pdf_details) to return, per output sample,
  slope -- (b1 - b0) / (c1 - c0) of the CDF interval the sample falls in (0 where c1 == c0): b = b0 + (u - c0) slope, so that an error
           of 2^-24 in u, c0 or c1 is one of 2^-24 slope in b; spacing bins are judged in mode "scaled" with scale 1 + slope;
  near  -- u lies within 64 x 2^-24 of a knot c_k > 0 that adjoins a flat run of the CDF (an interval no wider than 2^-22, which
           float32 may store as zero width).  There the output jumps by whole bins when u crosses the knot, and float32 and
           float64 may legitimately stand on different sides.  These samples are left out; CAP is the share that may be.  The knot
           c_0 = 0 is exact in every precision and u reaches it only as an exact 0, so samples there stay in: they are where
           searchsorted's side shows (tests/test_samplers_cpu.py).

Users: tests/test_samplers_cpu.py (the rule against a float32 emulation and its planted faults; the cap on every case) and
tests/test_samplers_gpu.py (the kernels)."""
import math

import torch

from oracle import cpu_ref
from tests import field_maths_reference as FM
from tests.helpers import default_dtype

f32, f64 = torch.float32, torch.float64
EPS = 2.0 ** -24
NEAR = 64 * EPS       # distance of u to a flat-run knot below which the sample is left out
FLAT = 2.0 ** -22     # a CDF interval this narrow may round to zero width in float32 (two knots below 1, half an ulp each, twice over)
CAP = 0.005           # at most this share of a case's samples may be left out
TAN = 0.25            # the reflect levels' reciprocal spacing (reflect_sampling_nerf_model.py)
R_SMALL, LIVE = 67, 41
U_LAST = 1.0 - 2.0 ** -24  # the largest float32 below 1


# ---------------------------------------------------------------------------------------------- inputs
def rays(kind, R, seed):
    """Per-ray near / far [R] float32 and the spacing's tan.  reciprocal: near 0, far log-uniform over [0.5, 200] with both ends
    present, tan 0.25 (the reflect levels); uniform: near in [0.05, 2], far = near + [0.5, 5.5]."""
    g = torch.Generator().manual_seed(seed)
    if kind == "reciprocal":
        near = torch.zeros(R, dtype=f64)
        far = 10.0 ** (math.log10(0.5) + (math.log10(200.0) - math.log10(0.5)) * torch.rand(R, generator=g, dtype=f64))
        far[0] = 0.5
        if R > 1:
            far[1] = 200.0
        return near.float(), far.float(), TAN
    near = 0.05 + 1.95 * torch.rand(R, generator=g, dtype=f64)
    far = near + 0.5 + 5.0 * torch.rand(R, generator=g, dtype=f64)
    return near.float(), far.float(), 1.0


def ray_classes(kind, fars):
    """Classes by spacing kind and decade of far -> (class index [R], names)."""
    dec = torch.floor(torch.log10(fars.double())).long()
    lo = int(dec.min())
    return dec - lo, [f"{kind}_far_1e{d}" for d in range(lo, int(dec.max()) + 1)]


def _spaced_cases():
    c = []
    for kind in ("uniform", "reciprocal"):
        c += [(kind, R_SMALL, S, jit, None) for S in (1, 2, 63, 128) for jit in (False, True)]
        c += [(kind, R_SMALL, 63, True, LIVE), (kind, R_SMALL, 2, True, 0)]
        c += [(kind, 4099, 128, True, 4097)]  # 528,771 elements against 2048 x 256 threads: the stride loop
    return c


SPACED_CASES = _spaced_cases()  # (kind, R, S, jitter, device-side count or None)


def spaced_id(c):
    return f"{c[0]}-R{c[1]}-S{c[2]}{'-jitter' if c[3] else ''}{'' if c[4] is None else f'-count{c[4]}'}"


_SPACED = {}


def spaced_case(kind, R, S, jitter, live=None):
    key = (kind, R, S, jitter)
    if key not in _SPACED:
        nears, fars, tan = rays(kind, R, 100 + S + R)
        g = torch.Generator().manual_seed(200 + S + R)
        t_rand = torch.rand(R, S + 1, generator=g) if jitter else None
        if jitter and R > 3:
            t_rand[2], t_rand[3] = 0.0, U_LAST
        cls, names = ray_classes(kind, fars)
        case = {"kind": kind, "tan": tan, "R": R, "S": S, "nears": nears, "fars": fars, "t_rand": t_rand, "cls": cls, "names": names}
        case["ref"], case["oracle"] = spaced_reference(case, f64), spaced_reference(case, f32)
        _SPACED[key] = case
    return _SPACED[key]


def spaced_reference(case, dtype):
    """cpu_ref.spaced_bins in `dtype` on the float32 inputs -> (spacing bins [R,S+1], euclidean bins [R,S+1])."""
    with default_dtype(dtype):
        t = case["t_rand"]
        sb, eb = cpu_ref.spaced_bins(case["kind"], case["tan"], case["nears"].to(dtype)[:, None], case["fars"].to(dtype)[:, None],
                                     case["S"], None if t is None else t.to(dtype))
        return sb.contiguous(), eb.contiguous()


def _pdf_cases():
    c = []
    for kind in ("uniform", "reciprocal"):
        for u in (False, True):
            c += [(kind, R_SMALL, si, so, 0.01, 0.0, u, None) for si, so in ((1, 1), (63, 64), (65, 33), (130, 129), (1024, 70))]
            c += [(kind, R_SMALL, si, so, 0.0, z, u, None) for si, so in ((65, 64), (130, 129)) for z in (0.5, 0.9)]
    c += [("reciprocal", R_SMALL, 65, 33, 0.01, 0.0, True, LIVE), ("reciprocal", R_SMALL, 65, 33, 0.0, 0.5, True, 0)]
    c += [("reciprocal", 16389, 7, 9, 0.01, 0.0, True, None)]  # 4096 blocks x 4 rays: the stride loop
    return c


PDF_CASES = _pdf_cases()  # (kind, R, s_in, s_out, histogram_padding, share of zeroed weights, u_rand, device-side count or None)


def pdf_id(c):
    return (f"{c[0]}-R{c[1]}-{c[2]}to{c[3]}-pad{c[4]:g}" + (f"-zero{c[5]:g}" if c[5] else "") + ("-urand" if c[6] else "")
            + ("" if c[7] is None else f"-count{c[7]}"))


_PDF = {}


def pdf_case(kind, R, s_in, s_out, pad, zero, u_rand, live=None):
    """Inputs of one rsn_sample_pdf call with its references.  Weights rand^4 with `zero` of them set to exact 0; ray 0 all-zero
    weights, ray 1 weights summing below 1e-5, ray 2 a leading and ray 3 a trailing run of zeros; input bins jittered; with u_rand,
    ray 2 and ray 4 draw exact zeros and ray 3 draws 1 - 2^-24 throughout."""
    key = (kind, R, s_in, s_out, pad, zero, u_rand)
    if key in _PDF:
        return _PDF[key]
    nears, fars, tan = rays(kind, R, 300 + s_in + s_out)
    g = torch.Generator().manual_seed(400 + 7 * s_in + s_out + int(100 * zero) + int(u_rand))
    w = torch.rand(R, s_in, generator=g) ** 4
    if zero:
        w = w * (torch.rand(R, s_in, generator=g) >= zero)
    run = max(1, s_in // 4)
    w[0] = 0.0
    w[1] = torch.rand(s_in, generator=g) * (1e-6 / s_in)
    w[2, :run] = 0.0
    w[3, s_in - run:] = 0.0
    with default_dtype(f32):
        t_in = torch.rand(R, s_in + 1, generator=g)
        sb_in = cpu_ref.spaced_bins(kind, tan, nears[:, None], fars[:, None], s_in, t_in)[0].contiguous()
    assert bool((sb_in[:, 1:] >= sb_in[:, :-1]).all())
    u = None
    if u_rand:
        u = torch.rand(R, s_out + 1, generator=g)
        u[2], u[3], u[4] = 0.0, U_LAST, 0.0
    cls, names = ray_classes(kind, fars)
    case = {"kind": kind, "tan": tan, "R": R, "s_in": s_in, "s_out": s_out, "pad": pad, "nears": nears, "fars": fars,
            "w": w.contiguous(), "sb_in": sb_in, "u_rand": u, "cls": cls, "names": names}
    case["ref"], case["oracle"] = pdf_reference(case, f64), pdf_reference(case, f32)
    case["details"] = pdf_details(case)
    if R > 1000:
        _PDF.clear()  # one big case at a time
    _PDF[key] = case
    return case


def pdf_reference(case, dtype):
    """cpu_ref.pdf_bins in `dtype` on the float32 inputs -> (spacing bins [R,s_out+1], euclidean bins [R,s_out+1])."""
    with default_dtype(dtype):
        u = case["u_rand"]
        sb, eb = cpu_ref.pdf_bins(case["kind"], case["tan"], case["nears"].to(dtype)[:, None], case["fars"].to(dtype)[:, None],
                                  case["w"].to(dtype)[..., None], case["sb_in"].to(dtype), case["s_out"], None if u is None else u.to(dtype),
                                  histogram_padding=case["pad"])
        return sb.contiguous(), eb.contiguous()


def pdf_details(case):
    """The inverse CDF restated in fp64 -> {"bins": b0 + t (b1 - b0) [R,nb] (equal to pdf_reference's, asserted on the CPU),
    "slope": [R,nb], "near": bool [R,nb]} as the module docstring defines them."""
    w, sb = case["w"].double(), case["sb_in"].double()
    s_in, nb = case["s_in"], case["s_out"] + 1
    wp = w + case["pad"]
    wsum = wp.sum(-1, keepdim=True)
    short = torch.relu(1e-5 - wsum)
    pdf = (wp + short / s_in) / (wsum + short)
    cdf = torch.cat([torch.zeros(w.shape[0], 1, dtype=f64), torch.cumsum(pdf, -1).clamp(max=1.0)], -1)
    u = torch.linspace(0.0, 1.0 - 1.0 / nb, nb, dtype=f64).expand(w.shape[0], nb)
    u = (u + case["u_rand"].double() / nb if case["u_rand"] is not None else u + 1.0 / (2 * nb)).contiguous()
    idx = torch.searchsorted(cdf, u, right=True)
    below, above = (idx - 1).clamp(0, s_in), idx.clamp(0, s_in)
    c0, c1, b0, b1 = cdf.gather(-1, below), cdf.gather(-1, above), sb.gather(-1, below), sb.gather(-1, above)
    rising = c1 > c0
    den = torch.where(rising, c1 - c0, torch.ones_like(c0))
    slope = torch.where(rising, (b1 - b0) / den, torch.zeros_like(c0))
    t = torch.where(rising, (u - c0) / den, torch.zeros_like(c0)).clamp(0, 1)
    flat = (cdf[:, 1:] - cdf[:, :-1]) <= FLAT                       # interval k = [c_k, c_k+1]
    knot = torch.zeros_like(cdf, dtype=torch.bool)
    knot[:, 1:] |= flat
    knot[:, :-1] |= flat
    knot &= cdf > 0
    cnt = torch.cat([torch.zeros(w.shape[0], 1, dtype=torch.long), torch.cumsum(knot.long(), -1)], -1)
    lo = torch.searchsorted(cdf, (u - NEAR).contiguous(), right=False)
    hi = torch.searchsorted(cdf, (u + NEAR).contiguous(), right=True)
    near = (cnt.gather(-1, hi) - cnt.gather(-1, lo)) > 0
    return {"bins": b0 + t * (b1 - b0), "slope": slope, "near": near, "u": u}


# ---------------------------------------------------------------------------------------------- the rule
def excluded_share(case):
    near = case["details"]["near"]
    return float(near.sum()) / near.numel()


def _located(v, index, nb):
    """The Verdict's `point` is an index into the kept samples: name the ray and the sample instead."""
    for r in v.rows:
        r["ray"], r["sample"] = divmod(int(index[r["point"]]), nb)
    return v


def report(v):
    return "\n".join(f"[{r['label']}] {r['quantity']} {r['cls']}: kernel {r['got']:.3e} (ray {r['ray']}, sample {r['sample']}), "
                     f"fp32 oracle {r['oracle']:.3e}, bound {r['bound']:.3e}{'' if r['ok'] else '  <-- FAIL'}" for r in v.rows)


def _sorted_rows(label, sb, eb):
    """Output bins are non-decreasing along every ray -> list of failures."""
    out = []
    for name, t in (("spacing", sb), ("euclidean", eb)):
        bad = (t[:, 1:] < t[:, :-1]).nonzero()
        if bad.numel():
            out.append(f"{label}: {name} bins of ray {int(bad[0, 0])} decrease at sample {int(bad[0, 1]) + 1}")
    return out


def judge_spaced(label, case, sb, eb, live=None):
    """rsn_sample_spaced's two outputs [R,S+1] (host tensors) on the rays [:live] -> (verdicts, failures)."""
    live = case["R"] if live is None else live
    if live == 0:
        return [], []
    (rsb, reb), (osb, oeb) = case["ref"], case["oracle"]
    cls = case["cls"][:live]
    nb = case["S"] + 1
    index = torch.arange(live * nb)
    vs = [_located(FM.compare(label, "spaced spacing bins", sb[:live].reshape(-1, 1), rsb[:live].reshape(-1, 1), osb[:live].reshape(-1, 1),
                              torch.zeros(live * nb, dtype=torch.long), ["all"], mode="abs"), index, nb),
          _located(FM.compare(label, "spaced euclidean bins", eb[:live].reshape(-1, 1), reb[:live].reshape(-1, 1), oeb[:live].reshape(-1, 1),
                              cls.repeat_interleave(nb), case["names"], mode="rel"), index, nb)]
    return vs, _sorted_rows(label, sb[:live], eb[:live])


def euclid_of(case, bins, dtype):
    """cpu_ref's map from spacing bins to Euclidean bins in `dtype`, on the case's float32 near / far."""
    with default_dtype(dtype):
        fn, fn_inv = cpu_ref.spacing_fns(case["kind"], case["tan"])
        s_near, s_far = fn(case["nears"].to(dtype))[:, None], fn(case["fars"].to(dtype))[:, None]
        b = bins.to(dtype)
        return fn_inv(b * s_far + (1 - b) * s_near)


def euclid_slope(case, bins):
    """|d euclidean / d spacing| of cpu_ref's map at `bins`, in fp64: far - near for the uniform spacing,
    (s_far - s_near) / (tan (1 - x)^2) at x = b s_far + (1 - b) s_near for the reciprocal one."""
    with default_dtype(f64):
        fn, _ = cpu_ref.spacing_fns(case["kind"], case["tan"])
        s_near, s_far = fn(case["nears"].double())[:, None], fn(case["fars"].double())[:, None]
        b = bins.double()
        if case["kind"] == "uniform":
            return (s_far - s_near).abs().expand_as(b)
        x = b * s_far + (1 - b) * s_near
        return (s_far - s_near).abs() / (case["tan"] * (1 - x) ** 2)


def judge_pdf(label, case, sb, eb, live=None):
    """rsn_sample_pdf's two outputs [R,s_out+1] (host tensors) on the rays [:live] -> (verdicts, failures, share left out).
    Spacing bins: scaled by 1 + slope.  Euclidean bins, twice, per spacing kind and decade of far.  Against cpu_ref.pdf_bins in fp64
    they are scaled by |e| + (1 + slope) |de/db|: e = map(b) carries the map's own relative error and the spacing bin's error, which
    is 2^-24 (1 + slope) in size, times the map's derivative (euclid_slope).  Errors relative to |e| alone cannot be held per case:
    a class has two to thirty rays in a case, and whether the float32 oracle met its steepest sample with an unlucky rounding is
    chance (its worst relative error of one class runs from 1e-7 to 1e-5 over the cases of this file).  And the map alone -- the
    fp64 map of the spacing bins the kernel itself wrote, relative, against the oracle's error on its own bins -- which no slope
    enters."""
    live = case["R"] if live is None else live
    if live == 0:
        return [], [], 0.0
    sb, eb = sb[: case["R"]], eb[: case["R"]]  # the buffers under test may be longer than the case
    (rsb, reb), (osb, oeb) = case["ref"], case["oracle"]
    d = case["details"]
    nb = case["s_out"] + 1
    keep = ~d["near"][:live].reshape(-1)
    index = keep.nonzero().flatten()
    share = 1.0 - index.numel() / keep.numel()
    failures = [] if share <= CAP else [f"{label}: {share:.4%} of the samples are near a flat-run knot, the cap is {CAP:.2%}"]
    pick = lambda t: t[:live].reshape(-1)[index].reshape(-1, 1)  # noqa: E731
    cls, names = case["cls"][:live].repeat_interleave(nb)[index], case["names"]
    vs = [_located(FM.compare(label, "pdf spacing bins", pick(sb), pick(rsb), pick(osb), torch.zeros(index.numel(), dtype=torch.long), ["all"],
                              mode="scaled", scale=1.0 + pick(d["slope"])), index, nb)]
    scale = pick(reb).abs() + (1.0 + pick(d["slope"])) * pick(euclid_slope(case, rsb))
    vs.append(_located(FM.compare(label, "pdf euclidean bins", pick(eb), pick(reb), pick(oeb), cls, names, mode="scaled", scale=scale), index, nb))
    vs.append(_located(FM.compare(label, "pdf euclidean map", pick(eb), pick(euclid_of(case, sb, f64)), pick(euclid_of(case, osb, f32)).double()
                                  - pick(euclid_of(case, osb, f64)) + pick(euclid_of(case, sb, f64)), cls, names, mode="rel"), index, nb))
    return vs, failures + _sorted_rows(label, sb[:live], eb[:live]), share
