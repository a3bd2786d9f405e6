"""fp64 references of the granular field evaluation -- explicit Gaussians (RSN_MODE_GAUSS: rsn_field_forward_gaussians and its
training variant) and a caller-supplied embedding (RSN_MODE_EMB: rsn_field_forward_embedding) -- restated on oracle/cpu_ref.py with
the parameters and the fp32 input BITS cast to double, the seeded inputs of those two modes, the rounded-operand forward whose
distance from fp64 is the noise scale of the plain-bf16 kernels, and fp64 forms of the standalone geometry kernels (contraction of
a full covariance, mirror reflection), and the rule the kernels' outputs are judged by (`judge`; its bounds are derived in the
docstring of tests/test_granular_gpu.py).  Host only.  Users: tests/test_granular_cpu.py (the restatement against the cpu_ref call
chain the suite already trusts, the exclusion cap on the reference alone, the mistakes the rule has to reject) and
tests/test_granular_gpu.py."""
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import field_maths_reference as FM
from tests.helpers import check_points, default_dtype

f32, f64 = torch.float32, torch.float64

HEAD_MIN = 1e-2       # pred_normals / n_dot_d divide by |raw normal head|: points whose fp64 norm is below this may be left out
GRAD_MIN_REL = 1e-3   # analytic normals divide by |d raw_density / d mean|: below this x the case's median may be left out
EXCLUDE_CAP = 0.005   # ... of at most this share of a case's points

# ---------------------------------------------------------------------------------------------- sizes
MI355X_CUS = 256
N_SMALL = 333  # 2 x 128 + 77: three 128-point tiles, the last with two full waves, one wave of 13 valid rows and one skipped wave


def n_loop128(cus):
    """Points for the kernels that launch min(tiles, cus) workgroups of 128-point tiles (exact fp32, bf16x6, bf16x3)."""
    return (2 * cus + 37) * 128 + 45


def n_loop256(cus):
    """Points for rsn_field_bf16_kernel<NB> (min(tiles, 2 cus) workgroups, 128-point tiles) and the ring kernel (256-point tiles,
    min(tiles, cus) workgroups)."""
    return (4 * cus + 37) * 128 + 45


# ---------------------------------------------------------------------------------------------- fields
# (layers, parameter width) -> seed of the Field's random init; the looping cases use (8, 256)
FIELD_SEEDS = {(8, 256): 131, (8, 64): 132, (4, 128): 133, (8, 200): 134}
SMALL_FIELDS = [(8, 64), (4, 128), (8, 256), (8, 200)]
_fields = {}


def make_field(layers, width, skips=None):
    """The package's Field on the host with its seeded random init (density bias shifted by +1 as in the suite's other field
    tests) -> (module, parameters by state_dict name, cpu_ref.FieldSpec).  Cached: the GPU file moves a deep copy to the device.
    skips: skip_connections other than the Field's default (tests/test_depth_skip_gpu.py); the seed then follows from the shape."""
    import reflect_sampling_nerf_amd as pkg

    key = (layers, width) if skips is None else (layers, width, tuple(skips))
    if key not in _fields:
        rng = torch.get_rng_state()
        torch.manual_seed(FIELD_SEEDS[key] if skips is None else 200 + 32 * layers + width + sum(skips))
        kw = {} if skips is None else {"skip_connections": tuple(skips)}
        f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=layers, base_mlp_layer_width=width, **kw)
        torch.set_rng_state(rng)
        with torch.no_grad():
            f.field_output_density.net.bias += 1.0
        P = {k: v.detach().clone() for k, v in f.state_dict().items()}
        fs = cpu_ref.FieldSpec(num_layers=layers, width=width) if skips is None else cpu_ref.FieldSpec(num_layers=layers, width=width, skip=tuple(skips))
        _fields[key] = (f.eval(), P, fs)
    return _fields[key]


def kernel_width(width):
    return next(w for w in (64, 128, 256) if width <= w)


# ---------------------------------------------------------------------------------------------- inputs
def _unit(g, n):
    return F.normalize(torch.randn(n, 3, generator=g, dtype=f64), dim=-1)


def gauss_inputs(N, seed, damped=True):
    """Explicit Gaussians in float32: means uniform in the radius-2 ball (the contraction's range), cov_diag log-uniform in
    [1e-4, 1e-2] (tests/test_multitile_gpu._rays' variance range: far smaller variances leave the frequencies up to 2^15 alive,
    whose fp32 phase is off by ~1e-2 rad -- fp32's limit, not a kernel's), unit view directions.  damped=False: cov_diag None."""
    g = torch.Generator().manual_seed(seed)
    means = _unit(g, N) * (2.0 * torch.rand(N, 1, generator=g, dtype=f64) ** (1.0 / 3.0))
    cov = 10.0 ** (-4.0 + 2.0 * torch.rand(N, 3, generator=g, dtype=f64))
    dirs = _unit(g, N)
    return {"means": means.float().contiguous(), "cov_diag": cov.float().contiguous() if damped else None,
            "view_dirs": dirs.float().contiguous()}


def emb_inputs(N, W, seed, P, fs):
    """A caller-supplied embedding [N, W] in float32: the trunk output (post-ReLU: non-negative, about half the entries exactly
    zero) of one float32 gauss_reference call on other means, so that the heads see the magnitudes of a real trunk output; the
    columns behind fs.width are the kernels' zero padding.  Plus unit view directions and a roughness in [0, 1.5]."""
    gi = gauss_inputs(N, seed + 1000)
    emb = gauss_reference(P, fs, gi["means"], gi["cov_diag"], None, dtype=f32)["embedding"].float()
    g = torch.Generator().manual_seed(seed)
    dirs = _unit(g, N).float().contiguous()
    rough = (1.5 * torch.rand(N, generator=g, dtype=f64)).float().contiguous()
    return {"embedding": F.pad(emb, (0, W - fs.width)).contiguous(), "view_dirs": dirs, "roughness": rough}


def input_sets(cus=MI355X_CUS):
    """Every input set tests/test_granular_gpu.py evaluates: (label, (layers, width), kind, N, seed).  kind: "gauss" (damped),
    "gauss_undamped" (cov_diag None), "emb"."""
    sets = [("loop gauss", (8, 256), "gauss", n_loop256(cus), 11), ("loop emb", (8, 256), "emb", n_loop256(cus), 12),
            ("train gauss", (8, 256), "gauss", n_loop128(cus), 13)]
    for k, key in enumerate(SMALL_FIELDS):
        sets += [(f"small gauss undamped {key}", key, "gauss_undamped", N_SMALL, 20 + k),
                 (f"small gauss {key}", key, "gauss", N_SMALL, 30 + k), (f"small emb {key}", key, "emb", N_SMALL, 40 + k)]
    return sets


def build_inputs(key, kind, N, seed):
    _, P, fs = make_field(*key)
    if kind == "emb":
        return emb_inputs(N, kernel_width(fs.width), seed, P, fs)
    return gauss_inputs(N, seed, damped=(kind == "gauss"))


# ---------------------------------------------------------------------------------------------- forward
def _cast(P, dt):
    return {k: v.detach().to(dt) for k, v in P.items()}


def _opt(t, dt, *shape):
    return None if t is None else t.detach().to(dt).reshape(*shape)


def _heads(P, fs, emb, view_dirs, roughness, want_diff_tint):
    """From the embedding on, in torch's default dtype: the five heads, SH-34 attenuated by `roughness` (None: softplus of the
    roughness head) and zeroed without directions, mlp_mid -> mid colour."""
    N = emb.shape[0]
    raw = cpu_ref.head(P, "field_output_density", emb).reshape(N)
    nh = cpu_ref.head(P, "field_output_normals", emb)
    pn = F.normalize(-F.normalize(nh, dim=-1), dim=-1)
    rr = cpu_ref.head(P, "field_output_roughness", emb)
    diff = torch.sigmoid(cpu_ref.head(P, "field_output_diff", emb))
    tint = torch.sigmoid(cpu_ref.head(P, "field_output_tint", emb))
    if view_dirs is None:
        sh, ndd = torch.zeros(N, 34), torch.zeros(N)
    else:
        rho = F.softplus(rr) if roughness is None else roughness.reshape(N, 1)
        sh, ndd = cpu_ref.integrated_sh(view_dirs, rho), (view_dirs * pn).sum(-1)
    mid = cpu_ref.mid_color(P, fs, sh, emb)
    return {"sigma": F.softplus(raw + fs.density_bias), "raw_density": raw, "embedding": emb, "pred_normals": pn, "n_dot_d": ndd,
            "diff": diff, "tint": tint, "roughness": torch.sigmoid(rr).reshape(N), "raw_roughness": rr.reshape(N),
            "color": diff + tint * mid if want_diff_tint else mid, "normal_head": nh, "mid": mid}


def gauss_reference(P, fs, means, cov_diag, view_dirs, dtype=f64):
    """RSN_MODE_GAUSS: cpu_ref.ipe -> density_from_encoding -> heads -> SH-34 attenuated by softplus of the roughness head (zeroed
    without directions) -> mid_color; color = diff + tint * mid, n_dot_d = 0 without directions.  -> dict of [N, ...] tensors:
    the outputs of rsn_field_outputs, `embedding`, and (for the exclusions) `normal_head`, `mid`."""
    with torch.no_grad(), default_dtype(dtype):
        Pd = _cast(P, dtype)
        enc = cpu_ref.ipe(fs, _opt(means, dtype, -1, 3), _opt(cov_diag, dtype, -1, 3))
        _, emb, _ = cpu_ref.density_from_encoding(Pd, fs, enc)
        return _heads(Pd, fs, emb, _opt(view_dirs, dtype, -1, 3), None, True)


def emb_reference(P, fs, embedding, view_dirs, roughness, want_diff_tint, dtype=f64):
    """RSN_MODE_EMB: the same from the heads on, on the first fs.width columns of `embedding`.  roughness given: it replaces the
    softplus in the SH attenuation; want_diff_tint false: color = mid (get_mid / get_low)."""
    with torch.no_grad(), default_dtype(dtype):
        emb = embedding.detach().to(dtype)[:, :fs.width]
        return _heads(_cast(P, dtype), fs, emb, _opt(view_dirs, dtype, -1, 3), _opt(roughness, dtype, -1), want_diff_tint)


def gauss_normals_reference(P, fs, means, cov_diag, chunk=16384):
    """-normalize(d raw_density / d mean) by fp64 autograd through the trunk and the density head only, the covariance a constant
    (reference field.py:125-127, 146-147).  -> (normals [N,3], |d raw_density / d mean| [N])."""
    with default_dtype(f64):
        Pd = _cast(P, f64)
        grads = []
        for lo in range(0, means.shape[0], chunk):
            m = means[lo:lo + chunk].detach().double().clone().requires_grad_(True)
            cd = None if cov_diag is None else cov_diag[lo:lo + chunk].detach().double()
            _, _, raw = cpu_ref.density_from_encoding(Pd, fs, cpu_ref.ipe(fs, m, cd))
            grads.append(torch.autograd.grad(raw.sum(), m)[0])
        g = torch.cat(grads)
        return -F.normalize(g, dim=-1), g.norm(dim=-1)


def rounded(fn, dtype):
    """`fn` (one of the references above) with the two operands of every GEMM -- every F.linear of oracle/cpu_ref.py: activations
    and weights; the bias starts the accumulator and is not rounded -- rounded to `dtype`, accumulation and everything else as
    before.  With bfloat16 its distance from the plain reference is the noise scale of the plain-bf16 kernels; with the
    reference's own dtype it is the reference."""
    def run(*args, **kwargs):
        linear = F.linear

        def q(x, w, b=None):
            return linear(x.to(dtype).to(x.dtype), w.to(dtype).to(w.dtype), b)

        F.linear = q
        try:
            return fn(*args, **kwargs)
        finally:
            F.linear = linear
    return run


def kept_points(label, norm, floor):
    """Points whose fp64 divisor `norm` [N] is at least `floor`; asserts that at most EXCLUDE_CAP of the points are left out."""
    keep = norm.double() >= floor
    out = int((~keep).sum())
    assert out <= EXCLUDE_CAP * keep.numel(), (f"{label}: {out} of {keep.numel()} points below {floor:.3e} "
                                               f"(cap {EXCLUDE_CAP:.1%}): change the seed or the head scale, not the cap")
    return keep


TOL = 1e-4        # test_gpu_parity.TOL
TOL_UNIT = 5e-4   # test_gpu_parity.TOL_UNIT
TOL_X3 = 2e-3     # test_field_level_split_bf16_modes: bf16x3
TOL_BF16 = 3e-2   # test_gpu_parity / test_multitile_gpu: plain bf16
SHAPES = {"sigma": (), "color": (3,), "pred_normals": (3,), "n_dot_d": (), "diff": (3,), "tint": (3,), "roughness": (),
          "raw_density": (), "raw_roughness": ()}
ALL = tuple(SHAPES)
REL = ("sigma", "raw_density", "raw_roughness", "embedding")
UNIT = ("pred_normals", "n_dot_d")


# ---------------------------------------------------------------------------------------------- the rule (bounds: tests/test_granular_gpu.py's docstring)
def tile_worst(e, tile):
    n = e.numel()
    nt = -(-n // tile)
    return torch.nn.functional.pad(e, (0, nt * tile - n)).reshape(nt, tile).amax(1).repeat_interleave(tile)[:n]


def judge(label, mode, got, ref, N, tile, grid, r16=None, allow=None):
    """Every output of `got` against the fp64 `ref` under the bounds of this file's docstring.  r16: the rounded-bf16 forward (plain
    bf16's unit vectors).  allow: {output: absolute allowance}, taken off the error before it is judged (cov_diag == NULL in bf16)."""
    base = {"f32": TOL, "bf16x6": TOL, "bf16x3": TOL_X3, "bf16": TOL_BF16}[mode]
    keep = kept_points(label, ref["normal_head"].norm(dim=-1), HEAD_MIN).double()
    print(f"[{label}] {int(N - keep.sum())} of {N} points left out of pred_normals / n_dot_d")
    for k, g in got.items():
        g, r = g.double().reshape(N, -1), ref[k].double().reshape(N, -1)
        if k == "embedding":  # the kernels' padded units are exact zeros
            assert bool((g[:, r.shape[1]:] == 0).all()), f"{label}: padded embedding columns are not exact zeros"
            g = g[:, :r.shape[1]]
        e = (g - r).abs().nan_to_num(nan=float("inf"))
        if allow:
            print(f"[{label}] {k}: worst error {float(e.max()):.3e} before the allowance of {allow[k]:.3e} is taken off")
            e = (e - allow[k]).clamp_min(0.0)
        if k in UNIT:
            e = e.amax(1) * keep
            if mode == "bf16":
                e16 = (r16[k].double().reshape(N, -1) - r).abs().amax(1) * keep
                bound = 4.0 * tile_worst(e16, tile) + 2.0 ** -8
                i = int(e.argmax())
                print(f"[{label}] {k}: worst {float(e[i]):.3e} where the rounded-bf16 forward's tile-worst is {float(bound[i] - 2.0 ** -8) / 4:.3e}; "
                      f"worst rounded-bf16 error anywhere {float(e16.max()):.3e}, kernel / rounded {float(e.max()) / max(float(e16.max()), 1e-300):.2f}")
                check_points(label, k + " / (4 x tile-worst rounded-bf16 error + 2^-8)", e / bound, 1.0, tile, grid)
            else:
                check_points(label, k, e, 10 * TOL_UNIT if mode == "bf16x3" else TOL_UNIT, tile, grid)
        elif k in REL:
            check_points(label, k + " / (1 + |ref|)", (e / (1.0 + r.abs())).amax(1), base, tile, grid)
        else:
            check_points(label, k, e.amax(1), base, tile, grid)


def judge_against_oracle(label, got, ref, ora, N):
    """field_maths_reference.compare on one class: worst |got - fp64| <= 4 x worst |float32 oracle - fp64| + one fp32 ulp."""
    keep = kept_points(label, ref["normal_head"].norm(dim=-1), HEAD_MIN)
    cls = torch.zeros(N, dtype=torch.long)
    for k, g in got.items():
        g, r, o = (t.reshape(N, -1)[:, :ref[k].reshape(N, -1).shape[1]] for t in (g, ref[k], ora[k]))
        rows = keep if k in UNIT else torch.ones(N, dtype=torch.bool)
        v = FM.compare(label, k, g[rows], r[rows], o[rows], cls[rows], ["all points"])
        print(v.report())
        assert v.ok, "\n" + v.report()


def oracle_allowance(ref, ora, N):
    """What cov_diag == NULL adds to a plain-bf16 bound: the fp32 rule's right-hand side, per output."""
    out = {}
    for k in ALL + ("embedding",):
        r, o = ref[k].double().reshape(N, -1), ora[k].double().reshape(N, -1)
        out[k] = FM.FACTOR * float((o - r).abs().max()) + FM.ULP * max(1.0, float(r.abs().max()))
    return out


# ---------------------------------------------------------------------------------------------- geometry
def contract(mean, cov, dtype=f64):
    """mip-NeRF-360 contraction of Gaussians with a FULL covariance [N,3,3] (reference field.py:98-119): mean' and J Sigma J^T,
    the diagonal clamped at 0; written out from the formula, not through cpu_ref.contract."""
    m, S = mean.detach().to(dtype), cov.detach().to(dtype).reshape(-1, 3, 3)
    n2 = (m * m).sum(-1, keepdim=True)
    n = n2.sqrt()
    outside = n > 1
    eye = torch.eye(3, dtype=dtype).expand(m.shape[0], 3, 3)
    outer = m[:, :, None] * m[:, None, :] / n2[:, :, None]
    J = torch.where(outside[:, :, None], ((2 * n[:, :, None] - 2) * (eye - outer) + eye) / n2[:, :, None], eye)
    Sc = J @ S @ J.transpose(-1, -2)
    d = torch.diagonal(Sc, dim1=-2, dim2=-1)
    Sc = Sc - torch.diag_embed(d) + torch.diag_embed(d.clamp_min(0))
    return torch.where(outside, (2 * n - 1) / n2 * m, m), Sc


def reflection(directions, normals, dtype=f64):
    """reference field.py:203-207: n . d and normalize(d - 2 (d . n) n) with F.normalize's 1e-12 floor; sums written out left
    to right, as one thread of rsn_reflection forms them."""
    d, n = directions.detach().to(dtype), normals.detach().to(dtype)
    dot = d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1] + d[:, 2] * n[:, 2]
    r = d - 2.0 * dot[:, None] * n
    ln = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]).sqrt().clamp_min(1e-12)
    return r / ln[:, None], dot


def reflection_inputs(seed=5, per_class=143):
    """rsn_reflection's input classes (float32): unit directions with unit normals, n = d, n = -d, n perpendicular to d, a zero
    normal, and directions of length 0.5 and 2.  7 x 143 = 1001 points: past 256 and no multiple of it."""
    g = torch.Generator().manual_seed(seed)
    names, ds, ns = [], [], []

    def add(name, d, n):
        names.append(name)
        ds.append(d)
        ns.append(n)

    k = per_class
    add("unit", _unit(g, k), _unit(g, k))
    d = _unit(g, k)
    add("n_is_d", d, d.clone())
    d = _unit(g, k)
    add("n_is_minus_d", d, -d)
    d = _unit(g, k)
    add("n_perp_d", d, F.normalize(torch.cross(d, _unit(g, k), dim=-1), dim=-1))
    add("zero_normal", _unit(g, k), torch.zeros(k, 3, dtype=f64))
    add("dir_half", 0.5 * _unit(g, k), _unit(g, k))
    add("dir_two", 2.0 * _unit(g, k), _unit(g, k))
    cls = torch.arange(len(names)).repeat_interleave(k)
    return {"d": torch.cat(ds).float().contiguous(), "n": torch.cat(ns).float().contiguous(), "cls": cls, "names": names}
