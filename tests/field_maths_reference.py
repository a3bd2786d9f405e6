"""fp64 references of the field kernels' per-sample arithmetic -- conical frustum -> contracted Gaussian, the integrated
positional encoding, the roughness-attenuated SH-34 encoding, the head activations and the hand-derived backward of the heads --
each taking the kernel's own fp32 inputs as exact numbers, the inputs that span the domain of that arithmetic, and the one rule
its rows are judged by.  Users: tests/test_field_maths_cpu.py (the references against oracle/cpu_ref.py in float32, and the
mutations the rule has to reject) and tests/test_field_maths_gpu.py (the rows the training kernels write before any GEMM reads
them).  Every function takes a dtype: float64 is the reference, float32 the oracle whose own error sets the bound."""
import math

import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests.helpers import default_dtype

S = 5               # samples per ray
ULP = 2.0 ** -23    # one fp32 ulp of a value of magnitude 1
FACTOR = 4.0        # the kernels and torch make the same roundings per formula, in another order
AREA_EXPONENTS = tuple(range(-10, -1))  # pixel-area decades [1e-10, 1e-9) .. [1e-2, 1e-1)
UNIT_EPS = (1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3)


# ---------------------------------------------------------------------------------------------- inputs
def _unit(g, n):
    return F.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)


def _generic(g, n):
    """cpu_ref.synthetic_rays' camera shell."""
    o = _unit(g, n) * 4.0 + 0.05 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    return o, F.normalize(-o + 0.3 * torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)


def _jittered(g, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, S + 1, generator=g, dtype=torch.float64).sort(dim=1).values


def _log_bins(g, n, e_lo, e_hi):
    return 10.0 ** (e_lo + (e_hi - e_lo) * torch.rand(n, S + 1, generator=g, dtype=torch.float64).sort(dim=1).values)


def build_inputs(seed=1, n_area=40, n_bins=24, n_axis=8, n_len=16):
    """Rays of every input class, concatenated: origins / directions [R,3], pixel_area [R], euclid_bins [R,S+1] in float32,
    `ray_class` [R] (index into `names`).  All classes are finite in the reference: no bin has t0 == t1 == 0."""
    g = torch.Generator().manual_seed(seed)
    names, parts = [], []

    def add(name, o, d, pa, eb):
        names.append(name)
        parts.append((o, d, pa, eb, torch.full((o.shape[0],), len(names) - 1, dtype=torch.long)))

    mid_area = lambda n: 10.0 ** (-6.0 + 2.0 * torch.rand(n, generator=g, dtype=torch.float64))  # noqa: E731
    # pixel area, one decade each: from the top frequency undamped to the lowest one damped to zero
    for e in AREA_EXPONENTS:
        o, d = _generic(g, n_area)
        eb = _jittered(g, n_area, 2.0, 6.0)
        eb[:, 1], eb[:, 3] = eb[:, 0], eb[:, 2]  # samples 0 and 2 have no extent along the ray: the area alone sets their damping
        add(f"area_1e{e}", o, d, 10.0 ** (e + torch.rand(n_area, generator=g, dtype=torch.float64)), eb)
    # bins
    o, d = _generic(g, n_bins)
    eb = _jittered(g, n_bins, 0.0, 6.0)
    eb[:, 0] = 0.0
    eb[:, 1:] += 1e-3  # t1 > 0
    add("t0_zero", o, d, mid_area(n_bins), eb)
    o, d = _generic(g, n_bins)
    eb = _jittered(g, n_bins, 2.0, 6.0)
    eb[:, 3] = eb[:, 2]
    add("zero_width", o, d, mid_area(n_bins), eb)
    o, d = _generic(g, n_bins)
    eb = 250.0 * (0.9 + 0.2 * torch.rand(n_bins, 1, generator=g, dtype=torch.float64)) + torch.cumsum(
        10.0 ** (-3.0 + torch.rand(n_bins, S + 1, generator=g, dtype=torch.float64)), dim=1)
    add("thin_250", o, d, mid_area(n_bins), eb)
    o, d = _generic(g, n_bins)
    eb = _log_bins(g, n_bins, -2.0, 3.0)
    eb[:, -1] = 1e3
    add("far_1e3", o, d, mid_area(n_bins), eb)
    # sample means just inside and just outside |mean| = 1 (the contraction's branch): a ray along u that passes the origin at
    # distance b, thin bins centred where it enters the sphere of radius 1 + eps
    n = n_bins
    u = _unit(g, n)
    w = F.normalize(torch.cross(u, _unit(g, n), dim=-1), dim=-1)
    b = 0.2 + 0.6 * torch.rand(n, 1, generator=g, dtype=torch.float64)
    eps = torch.tensor([UNIT_EPS[i % len(UNIT_EPS)] for i in range(n)], dtype=torch.float64)[:, None]
    tc = 4.0 - torch.sqrt((1.0 + eps) ** 2 - b * b)
    add("unit_sphere", -4.0 * u + b * w, u, mid_area(n), tc + (torch.arange(S + 1, dtype=torch.float64) - 0.5 * S) * 1e-3)
    # directions along +-x, +-y, +-z with the origin on the same axis: the SH poles, and mean mean^T / |mean|^2 == d d^T
    for a, ax in enumerate("xyz"):
        d = torch.zeros(n_axis, 3, dtype=torch.float64)
        d[:, a] = torch.tensor([1.0, -1.0] * (n_axis // 2), dtype=torch.float64)
        eb = _jittered(g, n_axis, 2.0, 6.0)
        eb[n_axis // 2:] = _log_bins(g, n_axis - n_axis // 2, -1.0, 2.5)
        add(f"axis_{ax}", -4.0 * d, d, mid_area(n_axis), eb)
    for name, ln in (("dir_half", 0.5), ("dir_two", 2.0)):
        o, d = _generic(g, n_len)
        add(name, o, ln * d, mid_area(n_len), _jittered(g, n_len, 2.0, 6.0))
    o, d, pa, eb, rc = (torch.cat([p[i] for p in parts]) for i in range(5))
    return {"o": o.float(), "d": d.float(), "pa": pa.float(), "eb": eb.float().contiguous(), "ray_class": rc, "names": names}


def build_inf_inputs(seed=2, per_decade=12):
    """get_inf_color's inputs: unit directions (the six poles among them) and sqradius over 1e-8 .. 1e2, a class per decade."""
    g = torch.Generator().manual_seed(seed)
    exps = list(range(-8, 2))
    M = per_decade * len(exps)
    d = _unit(g, M)
    for i in range(6):
        d[i * per_decade] = 0.0
        d[i * per_decade, i % 3] = 1.0 if i < 3 else -1.0
    cls = torch.arange(len(exps)).repeat_interleave(per_decade)
    sq = 10.0 ** (torch.tensor(exps, dtype=torch.float64)[cls] + torch.rand(M, generator=g, dtype=torch.float64))
    sq[0], sq[-1] = 1e-8, 1e2
    return {"d": d.float(), "sq": sq.float(), "point_class": cls, "names": [f"sq_1e{e}" for e in exps]}


def point_class(inp):
    return inp["ray_class"].repeat_interleave(S)


def point_dirs(inp, dtype=torch.float64):
    return inp["d"].to(dtype).repeat_interleave(S, 0)


# ---------------------------------------------------------------------------------------------- Gaussian, IPE, SH
def gaussian(inp, dtype):
    """-> contracted mean [N,3], diagonal variance [N,3], |mean| before the contraction [N]: cpu_ref.gaussian_blob and
    cpu_ref.contract in `dtype` on the float32 inputs."""
    with default_dtype(dtype):
        eb = inp["eb"].to(dtype)
        mean, cov = cpu_ref.gaussian_blob(inp["o"].to(dtype), inp["d"].to(dtype), inp["pa"].to(dtype).reshape(-1, 1), eb[:, :-1], eb[:, 1:])
        mc, cc = cpu_ref.contract(mean, cov)
        return mc.reshape(-1, 3), torch.diagonal(cc, dim1=-2, dim2=-1).reshape(-1, 3), mean.norm(dim=-1).reshape(-1)


def inf_gaussian(inf, dtype):
    """cpu_ref.inf_color's Gaussian: mean = 2 d, variance = 0.6 sq (1 - d^2)."""
    d, sq = inf["d"].to(dtype), inf["sq"].to(dtype).reshape(-1, 1)
    return 2 * d, 0.6 * sq * (1.0 - d * d)


def frequencies():
    with default_dtype(torch.float32):
        return cpu_ref.frequencies(cpu_ref.FieldSpec())


def phases(mean32, freqs32):
    """The IPE's float32 phases [N,48] of the sine and of the cosine half, as include/rsn.h and cpu_ref.ipe state them:
    fl(fl(2 pi x) f) and that + fl32(pi / 2).  Their rounding (up to 0.1 rad at the top frequency) is the reference
    implementation's own behaviour, so the reference takes them as exact numbers."""
    assert mean32.dtype == torch.float32 and freqs32.dtype == torch.float32
    ph = ((torch.tensor(2 * math.pi, dtype=torch.float32) * mean32)[..., None] * freqs32).reshape(mean32.shape[0], -1)
    return ph, ph + torch.tensor(math.pi / 2, dtype=torch.float32)


def ipe_rows(mean32, var, freqs32, dtype, cosine="shifted_sine", damping_power=2):
    """The 96 encoded columns 0..95 in cpu_ref.ipe's order (columns 96..98 are the mean): sin in `dtype` of the float32 phase times
    exp(-0.5 v f^2) with the variance of `dtype`.  cosine / damping_power: the mutations of tests/test_field_maths_cpu.py."""
    ps, pc = phases(mean32, freqs32)
    f = freqs32.to(dtype)
    damp = torch.exp(-0.5 * (var.to(dtype)[..., None] * f ** damping_power).reshape(var.shape[0], -1))
    s = torch.sin(ps.to(dtype))
    c = torch.sin(pc.to(dtype)) if cosine == "shifted_sine" else torch.cos(ps.to(dtype))
    return torch.cat([damp * s, damp * c], dim=-1)


def sh_rows(dirs, raw_roughness, dtype, rho="softplus"):
    """cpu_ref.integrated_sh on the ray's direction and rho = softplus(raw roughness), as rsn_field_kernel.h uses it."""
    with default_dtype(dtype):
        r = raw_roughness.to(dtype).reshape(-1, 1)
        return cpu_ref.integrated_sh(dirs.to(dtype), F.softplus(r) if rho == "softplus" else torch.sigmoid(r))


# ---------------------------------------------------------------------------------------------- heads
def heads_forward(raw_density, heads, dirs, density_bias, dtype):
    """From the raw values: sigma = softplus(raw + bias), roughness = sigmoid(raw roughness), pred_normals =
    normalize(-normalize(head)) with F.normalize's 1e-12 clamps, n_dot_d = d . pred_normals."""
    with default_dtype(dtype):
        h = heads.to(dtype)
        pn = F.normalize(-F.normalize(h[:, :3], dim=-1), dim=-1)
        return {"sigma": F.softplus(raw_density.to(dtype).reshape(-1) + density_bias), "roughness": torch.sigmoid(h[:, 3]),
                "pred_normals": pn, "n_dot_d": (dirs.to(dtype) * pn).sum(-1)}


def heads_backward(fw, gin, density_bias, dtype):
    """All 16 columns of dz_heads and the 4 of dz_rgb from the upstream gradients `gin` and the forward values `fw`
    (raw_density [N], heads [N,8], diff / tint [N,3], dirs [N,3], pred_normals [N,3], n_dot_d [N], normals [N,3]).  The sigmoid
    columns are closed forms; the normal head's go through autograd of normalize(-normalize(.)) and d . n, with the fused per-ray
    losses sum_s w |n - pn|^2 and sum_s w max(0, n.d)^2 (gin: ray_pn_loss / ray_ori_loss [R], weights [N]), whose per-sample
    gradients the kernels form from the forward pred_normals / n_dot_d.
    -> (dz_heads [N,16], dz_rgb [N,4], scale [N] of the normal head's gradient: |G| / (|head| |-normalize(head)|), clamped as
    F.normalize clamps -- what the projected gradient is a cancelling difference of)."""
    with default_dtype(dtype):
        c = lambda t: t.detach().to(dtype)  # noqa: E731
        hd, d = c(fw["heads"]), c(fw["dirs"])
        N = hd.shape[0]
        ray = torch.arange(N) // S
        z = lambda k, *s: c(gin[k]).reshape(N, *s) if gin.get(k) is not None else torch.zeros(N, *s)  # noqa: E731
        gs, gcol, gpn, gnd, gr = z("sigma"), z("color", 3), z("pred_normals", 3), z("n_dot_d"), z("roughness")
        dz = torch.zeros(N, 16)
        dz[:, 0] = gs * torch.sigmoid(c(fw["raw_density"]).reshape(N) + density_bias)
        h = hd[:, :3].clone().requires_grad_(True)
        pn = F.normalize(-F.normalize(h, dim=-1), dim=-1)
        ndd = (d * pn).sum(-1)
        loss = (gpn * pn).sum() + (gnd * ndd).sum()
        if gin.get("ray_pn_loss") is not None:
            w = c(gin["weights"]).reshape(N)
            # d/d pn of w |n - pn|^2 at the forward pn: -2 w (n - pn_fwd); linear in pn so that the forward value is what is used
            loss = loss + (c(gin["ray_pn_loss"])[ray, None] * w[:, None] * -2.0 * (c(fw["normals"]) - c(fw["pred_normals"])) * pn).sum()
        if gin.get("ray_ori_loss") is not None:
            w = c(gin["weights"]).reshape(N)
            loss = loss + (c(gin["ray_ori_loss"])[ray] * w * 2.0 * torch.clamp(c(fw["n_dot_d"]).reshape(N), min=0.0) * ndd).sum()
        g_h, g_pn = torch.autograd.grad(loss, [h, pn])
        dz[:, 1:4] = g_h
        ln = hd[:, :3].norm(dim=-1).clamp_min(1e-12)
        scale = g_pn.norm(dim=-1) / ln / (hd[:, :3].norm(dim=-1) / ln).clamp_min(1e-12)
        dif, tin, mid = c(fw["diff"]), c(fw["tint"]), hd[:, 4:7]
        dz[:, 4:7] = gcol * (dif * (1.0 - dif))
        sr = torch.sigmoid(hd[:, 3])
        dz[:, 8] = gr * sr * (1.0 - sr)
        dz[:, 12:15] = gcol * mid * (tin * (1.0 - tin))
        rgb = torch.zeros(N, 4)
        rgb[:, :3] = gcol * tin * (mid * (1.0 - mid))
        return dz.detach(), rgb, scale.detach()


def make_gin(R, seed=3):
    """Upstream gradients of [R,S] samples with exact zeros among them, and the fused per-ray normal losses."""
    g = torch.Generator().manual_seed(seed)
    N = R * S
    drop = lambda t: t * (torch.rand(t.shape[0], generator=g) > 0.1).reshape(-1, *([1] * (t.dim() - 1)))  # noqa: E731
    return {"sigma": drop(torch.randn(N, generator=g)).reshape(R, S), "color": drop(torch.randn(N, 3, generator=g)).reshape(R, S, 3),
            "pred_normals": drop(torch.randn(N, 3, generator=g)).reshape(R, S, 3), "n_dot_d": drop(torch.randn(N, generator=g)).reshape(R, S),
            "roughness": drop(torch.randn(N, generator=g)).reshape(R, S), "ray_pn_loss": drop(torch.randn(R, generator=g)),
            "ray_ori_loss": drop(torch.randn(R, generator=g)), "weights": torch.rand(N, generator=g).reshape(R, S)}


# ---------------------------------------------------------------------------------------------- head variants
def _affine(P, name, vals, lo, hi):
    """Scale and shift a one-row head so that its raw values over the test's points run from lo to hi."""
    a = (hi - lo) / float(vals.max() - vals.min())
    P[f"{name}.net.weight"] = P[f"{name}.net.weight"] * a
    P[f"{name}.net.bias"] = P[f"{name}.net.bias"] * a + (lo - a * float(vals.min()))


DENSITY_SPAN = (-26.0, 32.0)    # raw_density + density_bias: both ends of the softplus, and its x > 20 branch
ROUGHNESS_SPAN = (-30.0, 30.0)  # raw roughness: rho = softplus from ~0 to 30 (every SH band damped to 0)


def make_variants(P, fs, inp):
    """Parameter sets whose raw head values span the activations' domains over the points of `inp` (measured on an fp64 forward
    of the trunk): "wide" (density and roughness heads stretched), "zero_normals" (wide, normal head zero), "tiny_normals" (wide,
    normal head with norms spread over 1e-10 .. 1e-6), "const_roughness" (roughness head weight zero: rho is the same number whatever
    the GEMMs' arithmetic).  -> {name: parameters}, and the fp64 raw values of each: (raw_density [N], heads [N,8] without mid)."""
    def raw(Pv):
        with torch.no_grad(), default_dtype(torch.float64):
            P64 = {k: v.double() for k, v in Pv.items()}
            eb = inp["eb"].double()
            lv = cpu_ref.field_level(P64, fs, inp["o"].double(), inp["d"].double(), inp["pa"].double().reshape(-1, 1), eb,
                                     training=False, want_normals=False)
            emb = lv["emb"].reshape(-1, fs.width)
            hd = torch.zeros(emb.shape[0], 8)
            hd[:, :3] = cpu_ref.head(P64, "field_output_normals", emb)
            hd[:, 3] = lv["rough_raw"].reshape(-1)
            hd[:, 4:7] = lv["mid"].reshape(-1, 3)
            return cpu_ref.head(P64, "field_output_density", emb).reshape(-1), hd, lv

    rd, hd, _ = raw(P)
    wide = {k: v.clone() for k, v in P.items()}
    _affine(wide, "field_output_density", rd, DENSITY_SPAN[0] - fs.density_bias, DENSITY_SPAN[1] - fs.density_bias)
    _affine(wide, "field_output_roughness", hd[:, 3], *ROUGHNESS_SPAN)
    out = {"wide": wide}
    out["zero_normals"] = {k: (torch.zeros_like(v) if "field_output_normals" in k else v.clone()) for k, v in wide.items()}
    # the normal head as (1, 0.5, -0.3) x a (u - median u), u the default roughness head's raw value: zero in the middle of the
    # points' distribution, so that the norms run from 9e-7 down through every decade to 1e-10 and a few points below it
    tiny = {k: v.clone() for k, v in wide.items()}
    u, wr, br = raw(P)[1][:, 3], P["field_output_roughness.net.weight"], P["field_output_roughness.net.bias"]
    a = 7.5e-7 / float((u - u.median()).abs().max())
    cj = torch.tensor([1.0, 0.5, -0.3], dtype=torch.float64)
    tiny["field_output_normals.net.weight"] = (cj[:, None] * (a * wr.double())).to(wr.dtype)
    tiny["field_output_normals.net.bias"] = (cj * (a * (br.double() - float(u.median())))).to(br.dtype)
    out["tiny_normals"] = tiny
    out["const_roughness"] = {k: (torch.zeros_like(v) if k == "field_output_roughness.net.weight" else v.clone()) for k, v in P.items()}
    return out, {k: raw(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------- the rule
class Verdict:
    def __init__(self, rows):
        self.rows = rows
        self.ok = all(r["ok"] for r in rows)

    def report(self):
        return "\n".join(
            f"[{r['label']}] {r['quantity']} {r['cls']}: kernel {r['got']:.3e} (point {r['point']}, column {r['column']}), "
            f"fp32 oracle {r['oracle']:.3e}, bound {r['bound']:.3e}{'' if r['ok'] else '  <-- FAIL'}" for r in self.rows)

    def worst(self):
        return max(r["got"] for r in self.rows)


def compare(label, quantity, got, ref, oracle, cls, names, mode="abs", scale=None, factor=FACTOR):
    """The rule for fp32 rows, per input class:  worst |got - ref| <= factor x worst |oracle - ref| + floor.
    got: the rows under test, ref: their fp64 reference, oracle: cpu_ref's float32 value of the same quantity on the same inputs.
    mode "abs": absolute errors, floor = one fp32 ulp of max(1, the class's largest |ref|); "rel": errors relative to |ref|
    element by element, floor 2^-23; "scaled": errors divided by the per-point `scale`, floor 2^-23.  A non-finite entry of
    `got` is an infinite error.  -> Verdict (per class: both errors, the bound, where the worst one is)."""
    N = ref.shape[0]
    ref = ref.detach().double().cpu().reshape(N, -1)
    got, oracle = (t.detach().double().cpu().reshape(N, -1) for t in (got, oracle))
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(oracle).all()), f"{label} {quantity}: non-finite reference"
    if mode == "rel":
        den = ref.abs().clamp_min(1e-300)
    elif mode == "scaled":
        den = scale.detach().double().cpu().reshape(N, 1).clamp_min(1e-300)
    else:
        den = torch.ones(N, 1, dtype=torch.float64)
    eg = ((got - ref).abs() / den).nan_to_num(nan=float("inf"), posinf=float("inf"))
    eo = (oracle - ref).abs() / den
    rows = []
    for k, name in enumerate(names):
        m = cls == k
        if not bool(m.any()):
            continue
        idx = m.nonzero().flatten()
        e = eg[idx]
        flat = int(e.argmax())
        floor = ULP * (max(1.0, float(ref[idx].abs().max())) if mode == "abs" else 1.0)
        bound = factor * float(eo[idx].max()) + floor
        rows.append({"label": label, "quantity": quantity, "cls": name, "got": float(e.max()), "oracle": float(eo[idx].max()),
                     "bound": bound, "ok": float(e.max()) <= bound, "point": int(idx[flat // e.shape[1]]), "column": flat % e.shape[1]})
    return Verdict(rows)


BF16_REL, BF16_ABS = 2.0 ** -8, 1e-5  # one bf16 ulp; sincos_bf16 (3.9e-6 / 1.8e-6 on the CPU emulation) and v_exp_f32


def compare_bf16(label, quantity, got, ref, cls, names, extra=None):
    """The rule for the plain ring's bf16 rows, element by element: |got - ref| <= 2^-8 |ref| + 1e-5.  The Verdict's `got` is the
    worst |got - ref| - 2^-8 |ref| of the class (what the absolute term has to cover), its bound 1e-5 -- plus extra[class] for
    a class with a derived bound of its own."""
    N = ref.shape[0]
    ref, got = ref.detach().double().cpu().reshape(N, -1), got.detach().double().cpu().reshape(N, -1)
    ex = ((got - ref).abs() - BF16_REL * ref.abs()).nan_to_num(nan=float("inf"), posinf=float("inf"))
    rows = []
    for k, name in enumerate(names):
        idx = (cls == k).nonzero().flatten()
        if idx.numel() == 0:
            continue
        e = ex[idx]
        flat = int(e.argmax())
        bound = BF16_ABS + (extra or {}).get(name, 0.0)
        rows.append({"label": label, "quantity": quantity, "cls": name, "got": float(e.max()), "oracle": 0.0, "bound": bound,
                     "ok": float(e.max()) <= bound, "point": int(idx[flat // e.shape[1]]), "column": flat % e.shape[1]})
    return Verdict(rows)
