"""tests/field_maths_reference.py without a GPU: the input classes are what they claim to be, the fp64 references agree with
oracle/cpu_ref.py run in float32 under the rule the GPU rows are held to (with float32 restatements of the kernels' own
operation order in the kernels' place), and that rule rejects every mutation of the arithmetic it exists to catch."""
import pytest
import torch
import torch.nn.functional as F

from oracle import cpu_ref
from tests import field_maths_reference as R
from tests.helpers import default_dtype

f32, f64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def case():
    fs = cpu_ref.FieldSpec(num_layers=8, width=64)
    inp = R.build_inputs()
    cls, names = R.point_class(inp), inp["names"]
    variants, raws = R.make_variants(cpu_ref.init_params(fs, seed=7), fs, inp)
    c = {"fs": fs, "inp": inp, "cls": cls, "names": names, "freqs": R.frequencies(), "raws": raws}
    c["g64"], c["g32"] = R.gaussian(inp, f64), R.gaussian(inp, f32)
    c["gk"] = kernel_gaussian32(inp)
    c["inf"] = R.build_inf_inputs()
    return c


def kernel_gaussian32(inp):
    """frustum_to_contracted (csrc/rsn_field_common.h) in float32, operation by operation: the kernels' order of the formula whose
    torch order is cpu_ref.gaussian_blob / contract.  -> (mean [N,3], var [N,3])."""
    S = R.S
    o, d = inp["o"].repeat_interleave(S, 0), inp["d"].repeat_interleave(S, 0)
    pa = inp["pa"].repeat_interleave(S)
    t0, t1 = inp["eb"][:, :-1].reshape(-1), inp["eb"][:, 1:].reshape(-1)
    radius = pa.sqrt() / 1.7724538509055159
    mu, hw = (t0 + t1) / 2.0, (t1 - t0) / 2.0
    hw2, mu2 = hw * hw, mu * mu
    den = 3.0 * mu2 + hw2
    tmean = mu + (2.0 * mu * hw2) / den
    m = [o[:, c] + d[:, c] * tmean for c in range(3)]
    hw4 = hw2 * hw2
    var_t = hw2 / 3.0 - 0.26666666666666666 * ((hw4 * (12.0 * mu2 - hw2)) / (den * den))
    var_r = (radius * radius) * (mu2 / 4.0 + 0.4166666666666667 * hw2 - (0.26666666666666666 * hw4) / den)
    dmag = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).clamp_min(1e-10)
    eye = lambda i, j: 1.0 if i == j else 0.0  # noqa: E731
    Sm = [[var_t * (d[:, i] * d[:, j]) + var_r * (eye(i, j) - d[:, i] * (d[:, j] / dmag)) for j in range(3)] for i in range(3)]
    n2 = m[0] * m[0] + m[1] * m[1] + m[2] * m[2]
    n = n2.sqrt()
    out = n > 1.0
    n2s = torch.where(out, n2, torch.ones_like(n2))  # (the inside branch never divides)
    J = [[((2.0 * n - 2.0) * (eye(i, j) - m[i] * m[j] / n2s) + eye(i, j)) / n2s for j in range(3)] for i in range(3)]
    sc = (2.0 * n - 1.0) / n2s
    mean, var = [], []
    for i in range(3):
        acc = torch.zeros_like(n)
        for b in range(3):
            acc = acc + (J[i][0] * Sm[0][b] + J[i][1] * Sm[1][b] + J[i][2] * Sm[2][b]) * J[b][i]
        mean.append(torch.where(out, sc * m[i], m[i]))
        var.append(torch.where(out, acc, Sm[i][i]).clamp_min(0.0))
    assert all(t.dtype == f32 for t in mean + var)
    return torch.stack(mean, 1), torch.stack(var, 1)


def closed_backward32(fw, gin, bias, drop_projection=False, ori_always=False):
    """head_grad_inputs / head_grad_row (csrc/rsn_field_bwd_common.h) in float32: the hand-derived backward, with the two
    mutations of its normal chain.  -> (dz_heads [N,16], dz_rgb [N,4])."""
    hd, d = fw["heads"].float(), fw["dirs"].float()
    N = hd.shape[0]
    ray = torch.arange(N) // R.S
    g = {k: v.float() for k, v in gin.items()}
    gcol = g["color"].reshape(N, 3)

    def nbwd(x, gy):
        ln = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        y = x / ln
        return (gy - (0.0 if drop_projection else y * (y * gy).sum(-1, keepdim=True))) / ln

    dz = torch.zeros(N, 16)
    dz[:, 0] = g["sigma"].reshape(N) * torch.sigmoid(fw["raw_density"].float().reshape(N) + bias)
    w = g["weights"].reshape(N)
    G = g["pred_normals"].reshape(N, 3) + (g["ray_pn_loss"][ray] * w * -2.0)[:, None] * (fw["normals"].float() - fw["pred_normals"].float())
    ndd = fw["n_dot_d"].float().reshape(N)
    gd = g["n_dot_d"].reshape(N) + g["ray_ori_loss"][ray] * w * (2.0 * (ndd if ori_always else ndd.clamp_min(0.0)))
    G = G + gd[:, None] * d
    nraw = hd[:, :3]
    u = -(nraw / nraw.norm(dim=-1, keepdim=True).clamp_min(1e-12))
    dz[:, 1:4] = nbwd(nraw, -nbwd(u, G))
    dif, tin, mid = fw["diff"].float(), fw["tint"].float(), hd[:, 4:7]
    dz[:, 4:7] = gcol * (dif * (1.0 - dif))
    sr = torch.sigmoid(hd[:, 3])
    dz[:, 8] = g["roughness"].reshape(N) * sr * (1.0 - sr)
    dz[:, 12:15] = gcol * mid * (tin * (1.0 - tin))
    rgb = torch.zeros(N, 4)
    rgb[:, :3] = gcol * tin * (mid * (1.0 - mid))
    return dz, rgb


def _forward_values(case, variant):
    """Stand-ins for what a training forward leaves behind: the fp64 forward's raw values rounded to float32."""
    rd, hd, lv = case["raws"][variant]
    dirs = R.point_dirs(case["inp"], f32)
    fw = {"raw_density": rd.float(), "heads": hd.float(), "dirs": dirs, "diff": lv["diff"].reshape(-1, 3).float(),
          "tint": lv["tint"].reshape(-1, 3).float(),
          "normals": F.normalize(torch.randn(hd.shape[0], 3, generator=torch.Generator().manual_seed(5)), dim=-1)}
    fw.update({k: v for k, v in R.heads_forward(fw["raw_density"], fw["heads"], dirs, case["fs"].density_bias, f32).items()
               if k in ("pred_normals", "n_dot_d")})
    return fw


def _enc(case, mean32, var, dtype, **kw):
    return R.ipe_rows(mean32, var, case["freqs"], dtype, **kw)


def _oracle_ipe(case, mean32, var32):
    with default_dtype(f32):
        return cpu_ref.ipe(case["fs"], mean32, var32)[:, :96]


def _check(v):
    print(v.report())
    assert v.ok, "\n" + v.report()


# ---------------------------------------------------------------------------------------------- the inputs
def test_input_classes_are_present(case):
    inp, names = case["inp"], case["names"]
    Rn = inp["o"].shape[0]
    N = Rn * R.S
    assert N % 128 and N % 256 and N > 2000
    eb, rc = inp["eb"], inp["ray_class"]
    t0, t1 = eb[:, :-1], eb[:, 1:]
    assert bool((t1 >= t0).all()) and not bool(((t0 == 0) & (t1 == 0)).any()), "t0 == t1 == 0 is 0/0 in the reference too"
    rays = lambda n: rc == names.index(n)  # noqa: E731
    for e in R.AREA_EXPONENTS:
        pa = inp["pa"][rays(f"area_1e{e}")].double()
        assert pa.numel() and bool((pa >= 10.0 ** e * (1 - 1e-6)).all()) and bool((pa <= 10.0 ** (e + 1) * (1 + 1e-6)).all())
    assert bool(((t0[rays("t0_zero")][:, 0] == 0) & (t1[rays("t0_zero")][:, 0] > 0)).all())
    assert bool(((t0[rays("zero_width")] == t1[rays("zero_width")]) & (t0[rays("zero_width")] > 0)).any(dim=1).all())
    thin = rays("thin_250")
    assert bool((t0[thin] > 200).all()) and bool((t1[thin] < 300).all()) and bool(((t1 - t0)[thin] < 0.011).all())
    assert float(eb.max()) == 1e3 and float(eb.min()) == 0.0
    norm = case["g64"][2].reshape(Rn, R.S)[rays("unit_sphere")]
    assert bool(((norm > 1) & (norm < 1 + 1e-4)).any()) and bool(((norm < 1) & (norm > 1 - 1e-4)).any())
    for a, ax in enumerate("xyz"):
        d, o = inp["d"][rays(f"axis_{ax}")], inp["o"][rays(f"axis_{ax}")]
        off = [c for c in range(3) if c != a]
        assert bool((d[:, off] == 0).all()) and bool((o[:, off] == 0).all()) and {float(v) for v in d[:, a]} == {1.0, -1.0}
    for n, ln in (("dir_half", 0.5), ("dir_two", 2.0)):
        assert torch.allclose(inp["d"][rays(n)].norm(dim=-1), torch.tensor(ln), rtol=1e-6)
    # the damping exponent 0.5 v f^2 runs from the top frequency all but untouched (a zero-width bin at the smallest area) to the
    # lowest frequency gone (get_inf_color's job: a contracted frustum's variance stays below ~0.2, sqradius goes to 1e2)
    var, f = case["g64"][1], case["freqs"].double()
    ivar = R.inf_gaussian(case["inf"], f64)[1]
    lo, hi, hi_inf = float((0.5 * var * f[-1] ** 2).min()), float((0.5 * var * f[0] ** 2).max()), float((0.5 * ivar * f[0] ** 2).max())
    print(f"damping exponents: top frequency down to {lo:.2e}, lowest frequency up to {hi:.2e} (frustums) / {hi_inf:.2e} (inf)")
    assert lo < 0.01 and hi_inf > 25.0 and float((0.5 * var.amin(dim=1) * f[-1] ** 2).max()) > 1e3
    inf = case["inf"]
    assert float(inf["sq"].min()) == float(torch.tensor(1e-8)) and float(inf["sq"].max()) == 1e2 and bool((inf["d"].abs().amax(dim=1) == 1).sum() >= 6)


def test_head_variants_span_the_domains(case):
    fs = case["fs"]
    rd, hd, _ = case["raws"]["wide"]
    x = rd + fs.density_bias
    assert float(x.min()) < -17 and float(x.max()) > 20 and bool(((x > 15) & (x < 20)).any()) and bool(((x > 20) & (x < 25)).any())
    assert float(hd[:, 3].min()) <= -29.9 and float(hd[:, 3].max()) >= 29.9
    assert float(case["raws"]["zero_normals"][1][:, :3].abs().max()) == 0.0
    nn = case["raws"]["tiny_normals"][1][:, :3].norm(dim=-1)
    assert 0.0 < float(nn.min()) and float(nn.max()) < 1e-6
    assert all(bool(((nn >= lo) & (nn < 10 * lo)).any()) for lo in (1e-10, 1e-9, 1e-8, 1e-7)), "a decade of 1e-10 .. 1e-6 is empty"
    assert float(case["raws"]["const_roughness"][1][:, 3].std()) == 0.0
    ndd = _forward_values(case, "wide")["n_dot_d"]
    assert bool((ndd > 0).any()) and bool((ndd < 0).any())
    gin = R.make_gin(case["inp"]["o"].shape[0])
    assert all(bool((gin[k] == 0).any()) and bool((gin[k] != 0).any()) for k in gin if k != "weights")


def test_references_are_finite(case):
    """No reference value of any class is NaN or inf (compare() asserts the same of every reference it is handed)."""
    mean, var, norm = case["g64"]
    rows = [mean, var, norm, _enc(case, case["gk"][0], var, f64)]
    for variant in ("wide", "zero_normals", "tiny_normals"):
        fw = _forward_values(case, variant)
        rows.append(R.sh_rows(fw["dirs"], fw["heads"][:, 3], f64))
        rows += list(R.heads_forward(fw["raw_density"], fw["heads"], fw["dirs"], case["fs"].density_bias, f64).values())
        rows += list(R.heads_backward(fw, R.make_gin(case["inp"]["o"].shape[0]), case["fs"].density_bias, f64))
    im, iv = R.inf_gaussian(case["inf"], f64)
    rows += [im, iv, _enc(case, im.float(), iv, f64)]
    assert all(bool(torch.isfinite(t).all()) for t in rows)
    assert all(t.dtype == f64 for t in rows)


# ---------------------------------------------------------------------------------------------- reference against oracle
def test_gaussian_and_encoding_agree_with_the_oracle(case):
    """The kernels' order of the frustum formula (float32, on the CPU) and a float32 evaluation of ipe_rows in the kernels' place:
    within the rule of the fp64 reference, the float32 oracle being cpu_ref.gaussian_blob / contract / ipe."""
    cls, names = case["cls"], case["names"]
    (m64, v64, _), (m32, v32, _), (mk, vk) = case["g64"], case["g32"], case["gk"]
    _check(R.compare("cpu", "mean", mk, m64, m32, cls, names))
    _check(R.compare("cpu", "ipe", _enc(case, mk, vk, f32), _enc(case, mk, v64, f64), _oracle_ipe(case, mk, v32), cls, names))
    # ipe_rows in float32 IS cpu_ref.ipe: the mutations below start from the oracle's own rows
    assert torch.equal(_enc(case, mk, v32, f32), _oracle_ipe(case, mk, v32))
    inf = case["inf"]
    im, iv64 = R.inf_gaussian(inf, f64)
    _, iv32 = R.inf_gaussian(inf, f32)
    ivk = (0.6 * inf["sq"].reshape(-1, 1)) * (1.0 - inf["d"] * inf["d"])
    _check(R.compare("cpu", "inf ipe", _enc(case, im.float(), ivk, f32), _enc(case, im.float(), iv64, f64),
                     _oracle_ipe(case, im.float(), iv32), inf["point_class"], inf["names"]))


@pytest.mark.parametrize("variant", ["wide", "zero_normals", "tiny_normals"])
def test_heads_agree_with_the_oracle(case, variant):
    """The hand-derived backward in float32 in the kernels' place: within the rule of fp64 autograd, the oracle being the same
    autograd in float32; forward activations: float32 against fp64."""
    cls, names, bias = case["cls"], case["names"], case["fs"].density_bias
    fw = _forward_values(case, variant)
    gin = R.make_gin(case["inp"]["o"].shape[0])
    ref, ora = (R.heads_forward(fw["raw_density"], fw["heads"], fw["dirs"], bias, dt) for dt in (f64, f32))
    for k in ref:
        _check(R.compare("cpu " + variant, k, ora[k], ref[k], ora[k], cls, names, mode="rel" if k == "sigma" else "abs"))
    _check(R.compare("cpu " + variant, "sh", R.sh_rows(fw["dirs"], fw["heads"][:, 3], f32), R.sh_rows(fw["dirs"], fw["heads"][:, 3], f64),
                     R.sh_rows(fw["dirs"], fw["heads"][:, 3], f32), cls, names))
    (dz64, rgb64, sc), (dz32, rgb32, _) = (R.heads_backward(fw, gin, bias, dt) for dt in (f64, f32))
    dzk, rgbk = closed_backward32(fw, gin, bias)
    if variant == "zero_normals":
        assert bool(torch.isfinite(dzk).all()) and float(ref["pred_normals"].abs().max()) == 0.0
    _check(R.compare("cpu " + variant, "dz_heads[1:4]", dzk[:, 1:4], dz64[:, 1:4], dz32[:, 1:4], cls, names, mode="scaled", scale=sc))
    keep = [c for c in range(16) if c not in (1, 2, 3)]
    _check(R.compare("cpu " + variant, "dz_heads[other]", dzk[:, keep], dz64[:, keep], dz32[:, keep], cls, names))
    _check(R.compare("cpu " + variant, "dz_rgb", rgbk, rgb64, rgb32, cls, names))


# ---------------------------------------------------------------------------------------------- mutations
def _mutated(case, name):
    """-> (the fp32 oracle's rows with one mutation, their fp64 reference, the oracle's rows, compare()'s keywords)."""
    cls, names, bias = case["cls"], case["names"], case["fs"].density_bias
    (m64, v64, _), (m32, v32, _), (mk, vk) = case["g64"], case["g32"], case["gk"]
    if name in ("columns_swapped", "cosine_of_phase", "damping_f", "variance_1e-3"):
        ref, ora = _enc(case, mk, v64, f64), _oracle_ipe(case, mk, v32)
        if name == "columns_swapped":  # the two top frequencies of x: damped to zero in most classes
            got = ora.clone()
            got[:, [14, 15]] = ora[:, [15, 14]]
        elif name == "cosine_of_phase":
            got = _enc(case, mk, v32, f32, cosine="cos")
        elif name == "damping_f":
            got = _enc(case, mk, v32, f32, damping_power=1)
        else:
            got = _enc(case, mk, v32 * (1.0 + 1e-3), f32)
        return got, ref, ora, {}
    fw = _forward_values(case, "wide")
    if name in ("sh_band8_sign", "rho_sigmoid"):
        ref, ora = (R.sh_rows(fw["dirs"], fw["heads"][:, 3], dt) for dt in (f64, f32))
        if name == "sh_band8_sign":  # the m = 0 term of band 8: the only one of its band that is not zero at the poles
            got = ora.clone()
            got[:, 25] = -got[:, 25]
        else:
            got = R.sh_rows(fw["dirs"], fw["heads"][:, 3], f32, rho="sigmoid")
        return got, ref, ora, {}
    gin = R.make_gin(case["inp"]["o"].shape[0])
    (dz64, _, sc), (dz32, _, _) = (R.heads_backward(fw, gin, bias, dt) for dt in (f64, f32))
    dzk, _ = closed_backward32(fw, gin, bias, drop_projection=name == "projection_dropped", ori_always=name == "orientation_always")
    return dzk[:, 1:4], dz64[:, 1:4], dz32[:, 1:4], {"mode": "scaled", "scale": sc}


@pytest.mark.parametrize("name", ["columns_swapped", "cosine_of_phase", "damping_f", "variance_1e-3", "sh_band8_sign",
                                  "rho_sigmoid", "projection_dropped", "orientation_always"])
def test_the_rule_rejects_mutation(case, name):
    got, ref, ora, kw = _mutated(case, name)
    v = R.compare("mutation", name, got, ref, ora, case["cls"], case["names"], **kw)
    bad = [r for r in v.rows if not r["ok"]]
    print(f"{name}: rejected in {len(bad)} of {len(v.rows)} classes; worst {v.worst():.3e}")
    assert not v.ok, f"the rule passes the mutation {name}: the input classes are too narrow\n" + v.report()
    # and the unmutated oracle rows pass it
    assert R.compare("mutation", name + " (none)", ora, ref, ora, case["cls"], case["names"], **kw).ok


def test_the_bf16_rule_rejects_a_phase_error(case):
    """The plain ring's rule (one bf16 ulp + 1e-5) against the first item it exists for: a phase error of 1e-3 in its sine."""
    mk, v64 = case["gk"][0], case["g64"][1]
    ref = _enc(case, mk, v64, f64)
    ps, pc = R.phases(mk, case["freqs"])
    damp = torch.exp(-0.5 * (v64[..., None] * case["freqs"].double() ** 2).reshape(v64.shape[0], -1))
    shifted = torch.cat([damp * torch.sin(ps.double() + 1e-3), damp * torch.sin(pc.double() + 1e-3)], dim=-1)
    rounded = lambda t: t.to(torch.bfloat16)  # noqa: E731
    assert R.compare_bf16("cpu", "ipe", rounded(ref), ref, case["cls"], case["names"]).ok
    assert not R.compare_bf16("cpu", "ipe", rounded(shifted), ref, case["cls"], case["names"]).ok
