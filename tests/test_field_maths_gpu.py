"""The per-sample arithmetic of the training field kernels, read where the kernels leave it BEFORE any GEMM has run over it, against
fp64 (tests/field_maths_reference.py): the encoded rows saved.enc / saved.sh (conical frustum -> contracted Gaussian -> IPE; SH-34
attenuated by softplus roughness), the head activations beside their own pre-activations (sigma / raw_density, roughness and
pred_normals / saved.heads, n_dot_d), and the backward sweeps' dz_heads / dz_rgb, which head_grad_inputs / head_grad_row form from
the upstream gradients and forward values alone.  Every training kernel family is hit through set_mma_mode: at width 256 the
per-wave exact kernel (f32), the split ring (bf16x6) and the plain ring (bf16), at width 64 the per-wave kernels of all three modes.
The inputs span the arithmetic's domain (pixel areas over nine decades, t from 0 to 1e3, zero-width and thin bins, means either side
of the contraction's |mean| = 1, axis-aligned rays, directions of length 0.5 and 2; head parameters stretched so that the raw values
reach both ends of every activation), as rays of ONE launch per family and head variant, in poisoned buffers.

Out of scope: d_input and the analytic-normal sweep need the GEMM chain; they stay with tests/test_multitile_gpu.py.

Bounds.  None is measured on the code under test.  fp32 rows (f32, bf16x6; every row of the width-64 kernels): per input class,
worst |kernel - fp64| <= 4 x worst |cpu_ref in float32 - fp64| + one fp32 ulp of the quantity's scale (field_maths_reference.compare).
Where that bound comes out above 1e-5 it is fp32 in the reference's own formula, not slack:
  * IPE columns: the contracted variance is diag(J Sigma J) formed in fp32, so each entry carries ~2^-24 of the LARGEST entry of
    Sigma (the along-ray variance (t1 - t0)^2 / 12 of an ordinary bin, or the radial one at t = 1e3), while a coordinate the ray
    barely moves along has a variance v_c many decades smaller; the column exp(-f^2 v_c / 2) sin(.) is alive up to f^2 ~ 2 / v_c
    and multiplies that absolute error by f^2 / 2: |d enc| ~ 2^-24 max(Sigma) / v_c, 1e-3 where v_c / max(Sigma) = 1e-4 (classes
    area_1e-10, area_1e-9, t0_zero, far_1e3, dir_two; the fp32 oracle shows 1e-4 .. 5e-3 there, 2e-7 .. 1e-5 elsewhere).
  * SH column 25 (band 8, m = 0): 0.00909 (6435 z^8 - 12012 z^6 + 6930 z^4 - 1260 z^2 + 35) loses 2^-24 of the sum of its terms'
    magnitudes, 0.00909 x 26672 x 6e-8 = 1.4e-5 at |d| = 1 and 2^8 times that at |d| = 2.
bf16 rows (the plain ring's saved.enc / saved.sh): |got - ref| <= 2^-8 |ref| + 1e-5, one bf16 ulp plus sincos_bf16 (3.9e-6 sine,
1.8e-6 cosine on a float32 emulation over 4e6 arguments up to 8.3e5) and v_exp_f32.  fast_sigmoid / fast_softplus (plain ring):
twice the formula error with correctly rounded primitives, see FAST_SIGMOID / FAST_SOFTPLUS below.

Measured on MI355X: beside the constants below and in DESIGN.md section 4.14."""
import contextlib

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import train_graph
from tests import field_maths_reference as R
from tests.helpers import _POISON, _poisoned

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
FAMILIES = [("f32", 256), ("bf16x6", 256), ("bf16", 256), ("f32", 64), ("bf16x6", 64), ("bf16", 64)]
VARIANTS = ["wide", "zero_normals", "tiny_normals"]
# fast_sigmoid, relative to sigmoid(x): formula error with correctly rounded exp2 / rcp <= 0.89 x (2e-7 + 8e-8 |x|) on [-87, 87]
# (CPU); twice that expression for the hardware's 1-ulp v_exp / v_rcp.  Beyond |x| = 87 only a result in [0, 1.2e-38] is required
# (this file's raw values stay inside +-40).
# Measured on MI355X: 0.38 of this bound at worst (x = -23.4).
FAST_SIGMOID = lambda x: 2.0 * (2e-7 + 8e-8 * x.abs())  # noqa: E731
# fast_softplus, absolute: formula error <= 0.80 x (1.2e-7 + 2e-7 value) (CPU); twice that expression for v_exp / v_log.
# Measured on MI355X: 0.42 of this bound at worst (x = 12.2).
FAST_SOFTPLUS = lambda v: 2.0 * (1.2e-7 + 2e-7 * v)  # noqa: E731
# The fp32 rule (field_maths_reference.FACTOR = 4, floor 2^-23), measured on MI355X as kernel / float32 oracle / bound of the worst
# class; f32, bf16x6 at both widths and bf16 at width 64 give the same figures to two digits, their means are bit-equal:
#   mean 6.3e-7 / 6.3e-7 / 2.7e-6      IPE 5.0e-3 / 4.5e-3 / 1.8e-2 (far_1e3; at most 0.72 of a class's bound: area_1e-7, 1.5e-5 of
#   2.1e-5; 2e-7 .. 2e-6 in the classes without the variance effect)      IPE of get_inf_color 3.2e-7 / 2.6e-7 / 1.2e-6
#   SH 9.2e-4 / 9.2e-4 / 4.3e-3 (dir_two, values up to 2^8; at most 0.32 of a bound)      sigma (relative) 1.2e-7 / 1.2e-7 / 6.0e-7
#   roughness 8.7e-8 / 8.7e-8 / 4.7e-7      pred_normals 9.3e-8 / 9.3e-8 / 4.9e-7      n_dot_d 2.9e-7 / 2.9e-7 / 1.4e-6
#   dz_heads 1..3 (/ |G| / |head|) 5.2e-7 / 5.2e-7 / 2.2e-6 (at most 0.38 of a bound)      other dz_heads columns 2.8e-7 / 2.8e-7 / 1.5e-6      dz_rgb 8.4e-8 / 8.4e-8 / 4.6e-7
# The plain ring's bf16 rows (field_maths_reference.BF16_REL / BF16_ABS): every mean, IPE and SH entry within ONE bf16 ulp of fp64
# (the 1e-5 term is used by entries whose reference is ~0 only), except the IPE of the two classes below.
# Their IPE: 1.0e-3 (area_1e-10) and 4.2e-3 (far_1e3) beyond one bf16 ulp, 0.27 of 1e-5 + 4 x the float32 oracle's 1.3e-3 / 4.5e-3.


FP32_VARIANCE_CLASSES = ("area_1e-10", "far_1e3")


def _is_ring_bf16(mode, width):
    return mode == "bf16" and width == 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


_cases, _runs, _dead = {}, {}, []


@contextlib.contextmanager
def _launching():
    """GPU work of this file: once a launch has raised, no later test starts another one on the device."""
    if _dead:
        pytest.fail(f"an earlier launch of this file failed ({_dead[0]}): not launching again")
    try:
        yield
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        _dead.append(repr(e))
        raise


def _case(dev, width):
    """One field, its head variants and the inputs per width, shared by the three MMA modes."""
    if width not in _cases:
        torch.manual_seed(70 + width)
        f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=8, base_mlp_layer_width=width)
        P = {k: v.detach().clone() for k, v in f.state_dict().items()}
        fs = cpu_ref.FieldSpec(num_layers=8, width=width)
        inp = R.build_inputs()
        variants, _ = R.make_variants(P, fs, inp)
        Rn = inp["o"].shape[0]
        gin = R.make_gin(Rn)
        c = {"f": f.to(dev).train(), "fs": fs, "inp": inp, "variants": variants, "gin": gin, "R": Rn, "N": Rn * R.S,
             "cls": R.point_class(inp), "names": inp["names"], "freqs": R.frequencies(), "inf": R.build_inf_inputs(),
             "rays": (inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev)), "eb": inp["eb"].to(dev),
             "gin_dev": {k: v.contiguous().to(dev) for k, v in gin.items()},
             "g64": R.gaussian(inp, f64), "g32": R.gaussian(inp, f32)}
        assert c["N"] % 128 and c["N"] % 256
        assert [float(x) for x in f.field_desc().freqs] == c["freqs"].tolist()
        _cases[width] = c
    return _cases[width]


@contextlib.contextmanager
def _poisoned_allocators(f):
    """The package's own allocators, their buffers filled with NaN patterns before a kernel sees them."""
    a_saved, a_level, a_gout = f.alloc_saved, f.alloc_train_level, train_graph._alloc_gout

    def gout(field, N, dev, need_input):
        g, st = a_gout(field, N, dev, need_input)
        _poisoned(g)
        return g, st

    f.alloc_saved = lambda N, dev: _poisoned(a_saved(N, dev))
    f.alloc_train_level = lambda dev, *lead: _poisoned(a_level(dev, *lead))
    train_graph._alloc_gout = gout
    try:
        yield
    finally:
        del f.alloc_saved, f.alloc_train_level
        train_graph._alloc_gout = a_gout


def _load(c, mode, variant):
    f = c["f"]
    f.load_state_dict(c["variants"][variant])
    f.set_mma_mode(mode)
    return f


def _run(dev, mode, width, variant):
    """One evaluate_frustums_train + train_graph._field_backward on all input classes; everything the tests read, on the host."""
    key = (mode, width, variant)
    if key not in _runs:
        c = _case(dev, width)
        f = _load(c, mode, variant)
        with _launching(), _poisoned_allocators(f):
            lv = f.evaluate_frustums_train(*c["rays"], c["eb"], want_normals=True)
            go = train_graph._field_backward(f, c["rays"], c["eb"], lv, c["gin_dev"], True)
        N, lay = c["N"], f.train_layout()
        host = lambda t, *s: t.detach().cpu().reshape(N, *s)  # noqa: E731
        r = {"lay": lay, "enc": host(lv["saved"]["enc"], -1), "sh": host(lv["saved"]["sh"], -1), "heads": host(lv["saved"]["heads"], 8),
             "raw_density": host(lv["raw_density"]), "sigma": host(lv["sigma"]), "roughness": host(lv["roughness"]),
             "pred_normals": host(lv["pred_normals"], 3), "n_dot_d": host(lv["n_dot_d"]), "diff": host(lv["diff"], 3),
             "tint": host(lv["tint"], 3), "normals": host(lv["normals"], 3), "dz_heads": host(go["dz_heads"], 16),
             "dz_rgb": host(go["dz_rgb"], 4)}
        _runs[key] = r
    return _runs[key]


def _columns(label, rows, cmap, n_cols):
    """Rows in slot order -> [N, n_cols] in the reference's column order; every column mapped once, padding slots exact zeros."""
    rows, cmap = rows.float(), torch.tensor(cmap)
    live = (cmap >= 0).nonzero().flatten()
    assert sorted(cmap[live].tolist()) == list(range(n_cols)), f"{label}: the slot map does not cover the {n_cols} columns once"
    pad = rows[:, cmap < 0]
    assert bool((pad == 0).all()), f"{label}: {int((pad != 0).sum())} non-zero (or unwritten) padding entries"
    out = torch.empty(rows.shape[0], n_cols)
    out[:, cmap[live]] = rows[:, live]
    return out


def _check(v):
    print(v.report())
    assert v.ok, "\n" + v.report()


def _oracle_ipe(c, mean32, var32):
    with R.default_dtype(f32):
        return cpu_ref.ipe(c["fs"], mean32, var32)[:, :96]


def _kernel_means(dev, mode, width, r):
    """The float32 means the family's phases were formed from: its own saved columns 96..98 -- except on the plain ring, which
    saves them rounded to bf16; there the exact per-wave kernel's, formed by the same frustum_to_contracted."""
    if not _is_ring_bf16(mode, width):
        return _columns("enc", r["enc"], r["lay"]["enc_map"], 99)[:, 96:]
    r0 = _run(dev, "f32", width, "wide")
    return _columns("enc", r0["enc"], r0["lay"]["enc_map"], 99)[:, 96:]


# ---------------------------------------------------------------------------------------------- encodings
@pytest.mark.parametrize("mode,width", FAMILIES)
def test_encoded_rows_against_fp64(dev, mode, width):
    """saved.enc (99 mapped columns) and saved.sh (34) of a training forward; padding slots exact zeros."""
    c = _case(dev, width)
    r = _run(dev, mode, width, "wide")
    label, cls, names = f"{mode} {width}", c["cls"], c["names"]
    ring16 = _is_ring_bf16(mode, width)
    assert r["lay"]["narrow_dtype"] == (torch.bfloat16 if ring16 else f32) and r["enc"].dtype == r["lay"]["narrow_dtype"]
    enc = _columns(label + " enc", r["enc"], r["lay"]["enc_map"], 99)
    sh = _columns(label + " sh", r["sh"], r["lay"]["sh_map"], 34)
    (m64, v64, _), (m32, v32, _) = c["g64"], c["g32"]
    mean = _kernel_means(dev, mode, width, r)
    ref_ipe = R.ipe_rows(mean, v64, c["freqs"], f64)
    rough = r["heads"][:, 3]
    assert float(rough.min()) < -25 and float(rough.max()) > 25, f"{label}: raw roughness spans {float(rough.min())} .. {float(rough.max())}"
    dirs = R.point_dirs(c["inp"], f32)
    ref_sh = R.sh_rows(dirs, rough, f64)
    if ring16:
        _check(R.compare_bf16(label, "mean", enc[:, 96:], m64, cls, names))
        # the two classes whose fp32 variance error (the first derivation in this file's docstring) is above what one bf16 ulp
        # covers: their absolute term is 1e-5 plus the fp32 rows' bound, 4 x the float32 oracle's own error on the class
        eo = {r_["cls"]: r_["oracle"] for r_ in R.compare(label, "ipe", ref_ipe, ref_ipe, _oracle_ipe(c, mean, v32), cls, names).rows}
        extra = {k: R.FACTOR * eo[k] for k in FP32_VARIANCE_CLASSES}
        _check(R.compare_bf16(label, "ipe", enc[:, :96], ref_ipe, cls, names, extra=extra))
        _check(R.compare_bf16(label, "sh", sh, ref_sh, cls, names))
        return
    _check(R.compare(label, "mean", mean, m64, m32, cls, names))
    _check(R.compare(label, "ipe", enc[:, :96], ref_ipe, _oracle_ipe(c, mean, v32), cls, names))
    _check(R.compare(label, "sh", sh, ref_sh, R.sh_rows(dirs, rough, f32), cls, names))


def test_width_64_exact_and_split_rows_are_bit_equal(dev):
    """At width 64 the enc and sh rows of f32 and bf16x6 come from one kernel template.  The SH rows depend on the GEMMs through
    rho = softplus(raw roughness), so they are compared on a roughness head with zero weight (the raw value is the bias in both)."""
    a, b = _run(dev, "f32", 64, "wide"), _run(dev, "bf16x6", 64, "wide")
    assert torch.equal(a["enc"].view(torch.int32), b["enc"].view(torch.int32))
    a, b = _run(dev, "f32", 64, "const_roughness"), _run(dev, "bf16x6", 64, "const_roughness")
    assert torch.equal(a["heads"][:, 3], b["heads"][:, 3]) and float(a["heads"][:, 3].min()) == float(a["heads"][:, 3].max())
    assert torch.equal(a["enc"].view(torch.int32), b["enc"].view(torch.int32))
    assert torch.equal(a["sh"].view(torch.int32), b["sh"].view(torch.int32)) and float(a["sh"].abs().max()) > 0.1


# ---------------------------------------------------------------------------------------------- heads
def _beyond(got, ref, allowance):
    """`got` with the part of its error that `allowance` (elementwise, absolute) covers taken out: what is left is held to the fp32 rule."""
    e = got.double() - ref
    return ref + torch.sign(e) * (e.abs() - allowance).clamp_min(0.0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("mode,width", FAMILIES)
def test_heads_forward_and_backward_against_fp64(dev, mode, width, variant):
    """sigma, roughness, pred_normals, n_dot_d from the kernel's own raw values; all 16 columns of dz_heads and dz_rgb from the
    upstream gradients and the kernel's own forward values (fp64 autograd for the normal chain, fused per-ray losses included)."""
    c = _case(dev, width)
    r = _run(dev, mode, width, variant)
    label, cls, names, bias = f"{mode} {width} {variant}", c["cls"], c["names"], c["fs"].density_bias
    fast = _is_ring_bf16(mode, width)
    dirs = R.point_dirs(c["inp"], f32)
    x = r["raw_density"].double() + bias
    hn = r["heads"][:, :3].double().norm(dim=-1)
    print(f"[{label}] raw_density + bias {float(x.min()):.2f} .. {float(x.max()):.2f}, raw roughness {float(r['heads'][:, 3].min()):.2f} .. "
          f"{float(r['heads'][:, 3].max()):.2f}, |normal head| {float(hn.min()):.2e} .. {float(hn.max()):.2e}")
    assert float(x.min()) < -17 and float(x.max()) > 20 and bool(((x > 15) & (x < 20)).any()) and bool(((x > 20) & (x < 25)).any())
    assert float(r["heads"][:, 3].min()) < -25 and float(r["heads"][:, 3].max()) > 25
    assert bool((r["n_dot_d"] > 0).any()) == bool((r["n_dot_d"] < 0).any()) == (variant != "zero_normals")
    if variant == "zero_normals":
        assert float(hn.max()) == 0.0 and float(r["pred_normals"].abs().max()) == 0.0 and float(r["n_dot_d"].abs().max()) == 0.0
        assert bool(torch.isfinite(r["dz_heads"][:, 1:4]).all())
    if variant == "tiny_normals":  # (bf16 GEMMs move the norms below ~1e-8: only the ends of the spread are asserted there)
        assert 0.0 < float(hn.min()) < 1e-8 and float(hn.max()) < 1e-6
        assert mode == "bf16" or all(bool(((hn >= lo) & (hn < 10 * lo)).any()) for lo in (1e-10, 1e-9, 1e-8, 1e-7))
    # ---- forward
    ref, ora = (R.heads_forward(r["raw_density"], r["heads"], dirs, bias, dt) for dt in (f64, f32))
    if fast:
        e_sp = (r["sigma"].double() - ref["sigma"]).abs() / FAST_SOFTPLUS(ref["sigma"])
        e_sg = (r["roughness"].double() - ref["roughness"]).abs() / ref["roughness"] / FAST_SIGMOID(r["heads"][:, 3].double())
        print(f"[{label}] fast_softplus: worst error / bound {float(e_sp.max()):.3f} at x = {float(x[e_sp.argmax()]):.2f}; "
              f"fast_sigmoid: {float(e_sg.max()):.3f} at x = {float(r['heads'][e_sg.argmax(), 3]):.2f}")
        assert float(e_sp.max()) <= 1.0 and float(e_sg.max()) <= 1.0
    else:
        _check(R.compare(label, "sigma", r["sigma"], ref["sigma"], ora["sigma"], cls, names, mode="rel"))
        _check(R.compare(label, "roughness", r["roughness"], ref["roughness"], ora["roughness"], cls, names))
    _check(R.compare(label, "pred_normals", r["pred_normals"], ref["pred_normals"], ora["pred_normals"], cls, names))
    _check(R.compare(label, "n_dot_d", r["n_dot_d"], ref["n_dot_d"], ora["n_dot_d"], cls, names))
    # ---- backward
    fw = {k: r[k] for k in ("raw_density", "heads", "diff", "tint", "pred_normals", "n_dot_d", "normals")}
    fw["dirs"] = dirs
    (dz64, rgb64, sc), (dz32, rgb32, _) = (R.heads_backward(fw, c["gin"], bias, dt) for dt in (f64, f32))
    dz, unused = r["dz_heads"], [7, 9, 10, 11, 15]
    assert bool((dz[:, unused] == 0).all()) and bool((r["dz_rgb"][:, 3] == 0).all()), f"{label}: unused gradient columns are not exact zeros"
    g = {k: c["gin"][k].reshape(c["N"], -1).double() for k in ("sigma", "color", "pred_normals", "n_dot_d", "roughness")}
    assert all(bool((g[k] == 0).any()) for k in ("sigma", "color", "pred_normals", "n_dot_d", "roughness"))
    others = [0, 4, 5, 6, 8, 12, 13, 14]
    got = dz[:, others].double()
    if fast:  # the two columns through fast_sigmoid: |g| s d(x) for softplus' = s, |g| s d(x) (1 + d(x)) for s (1 - s)
        sx, sr = torch.sigmoid(x), torch.sigmoid(r["heads"][:, 3].double())
        dx, dr = FAST_SIGMOID(x), FAST_SIGMOID(r["heads"][:, 3].double())
        got[:, 0] = _beyond(got[:, 0], dz64[:, 0], g["sigma"][:, 0].abs() * sx * dx)
        got[:, 4] = _beyond(got[:, 4], dz64[:, 8], g["roughness"][:, 0].abs() * sr * dr * (1.0 + dr))
    _check(R.compare(label, "dz_heads[sigmoid columns]", got, dz64[:, others], dz32[:, others], cls, names))
    _check(R.compare(label, "dz_heads[1:4]", dz[:, 1:4], dz64[:, 1:4], dz32[:, 1:4], cls, names, mode="scaled", scale=sc))
    _check(R.compare(label, "dz_rgb", r["dz_rgb"], rgb64, rgb32, cls, names))


# ---------------------------------------------------------------------------------------------- get_inf_color, short counts
def _poison_or_zero(t):
    it, pattern = _POISON[t.dtype]
    w = t.contiguous().view(it)
    return bool(((w == pattern) | (w == 0)).all())


@pytest.mark.parametrize("mode,width", FAMILIES)
def test_inf_job_rows_and_rows_behind_the_count(dev, mode, width):
    """evaluate_reflect_train: the frustum level with a device-side ray count below its buffers (live rows written, their enc
    rows the bits of the full launch; rows behind the count: still poisoned, or zero) and the get_inf_color job (enc rows against mean = 2 d, var = 0.6 sq
    (1 - d^2) with sq over 1e-8 .. 1e2; sh rows exact zeros).  Then the backward with the same count."""
    c = _case(dev, width)
    full = _run(dev, mode, width, "wide")
    f = _load(c, mode, "wide")
    label, inf, S = f"{mode} {width}", c["inf"], R.S
    ring16 = _is_ring_bf16(mode, width)
    live_rays = c["R"] - 7
    n_dev = torch.tensor([live_rays], dtype=torch.int32, device=dev)
    M = inf["d"].shape[0]
    assert M < live_rays
    gin = {k: c["gin_dev"][k] for k in ("sigma", "color", "pred_normals", "n_dot_d", "roughness")}
    with _launching(), _poisoned_allocators(f):
        lv, _, inf_saved = f.evaluate_reflect_train(*c["rays"], c["eb"], n_dev, inf["sq"].to(dev), inf_directions=inf["d"].to(dev))
        go = train_graph._field_backward(f, c["rays"], c["eb"], lv, gin, True, n_dev=n_dev)
    live = live_rays * S
    rows = lv["saved"]["enc"].cpu().reshape(c["N"], -1)
    it = _POISON[rows.dtype][0]
    assert torch.equal(rows[:live].view(it), full["enc"][:live].view(it)), f"{label} saved.enc: live rows differ from the full launch"
    for k, t in [("saved." + k, lv["saved"][k]) for k in ("enc", "sh", "heads")] + [(k, lv[k]) for k in ("sigma", "pred_normals", "n_dot_d", "roughness")]:
        rows = t.cpu().reshape(c["N"], -1)
        assert bool(torch.isfinite(rows[:live].float()).all()), f"{label} {k}: unwritten live rows"
        assert _poison_or_zero(rows[live:]), f"{label} {k}: rows behind the device-side count were written"
    for k in ("dz_heads", "dz_rgb"):
        rows = go[k].cpu()
        assert bool(torch.isfinite(rows[:live]).all()) and _poison_or_zero(rows[live:]), f"{label} {k}: rows behind the count / live rows"
    # ---- get_inf_color
    lay = f.train_layout()
    enc = _columns(label + " inf enc", inf_saved["enc"].cpu(), lay["enc_map"], 99)
    sh = inf_saved["sh"].cpu().float()
    assert bool((sh == 0).all()), f"{label}: get_inf_color's sh rows are not exact zeros"
    m64, v64 = R.inf_gaussian(inf, f64)
    _, v32 = R.inf_gaussian(inf, f32)
    mean = (2 * inf["d"]).float()
    ref = R.ipe_rows(mean, v64, c["freqs"], f64)
    if ring16:
        _check(R.compare_bf16(label, "inf mean", enc[:, 96:], m64, inf["point_class"], inf["names"]))
        _check(R.compare_bf16(label, "inf ipe", enc[:, :96], ref, inf["point_class"], inf["names"]))
    else:
        assert torch.equal(enc[:, 96:], mean), f"{label}: get_inf_color's mean is not 2 d"
        _check(R.compare(label, "inf ipe", enc[:, :96], ref, _oracle_ipe(c, mean, v32), inf["point_class"], inf["names"]))
