"""tests/granular_reference.py on the host: the restatement of the two granular modes against the cpu_ref call chain that
test_gpu_parity.test_granular_field_api trusts (in float32, where both are the same arithmetic), the exclusion cap of
tests/test_granular_gpu.py on the reference alone (so that no GPU run can hide behind it), the rounded-operand forward, the rule of
the GPU file against the mistakes it exists to catch (a second loop iteration one row off, an unwritten ragged wave, ignored flags,
the wrong colour branch), and the argument errors of the three granular entry points that return before any launch (the library loads without a device)."""
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi
from reflect_sampling_nerf_amd._build import build_library
from tests import field_maths_reference as FM
from tests import granular_reference as G

f32, f64 = torch.float32, torch.float64
OUTPUTS = ("sigma", "raw_density", "embedding", "pred_normals", "n_dot_d", "diff", "tint", "roughness", "raw_roughness", "color")


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("key", G.SMALL_FIELDS)
def test_float32_references_equal_the_cpu_ref_call_chain(key):
    """gauss_reference / emb_reference in float32 against test_granular_field_api's calls, one by one."""
    _, P, fs = G.make_field(*key)
    N = 97
    gi = G.gauss_inputs(N, seed=3)
    m, cd, d = gi["means"], gi["cov_diag"], gi["view_dirs"]
    with torch.no_grad():
        sig, emb, raw = cpu_ref.density_from_encoding(P, fs, cpu_ref.ipe(fs, m, cd))
        pn = cpu_ref.pred_normals(P, emb)
        diff = torch.sigmoid(cpu_ref.head(P, "field_output_diff", emb))
        tint = torch.sigmoid(cpu_ref.head(P, "field_output_tint", emb))
        rr = cpu_ref.head(P, "field_output_roughness", emb)
        mid = cpu_ref.mid_color(P, fs, cpu_ref.integrated_sh(d, torch.nn.functional.softplus(rr)), emb)
        low = cpu_ref.mid_color(P, fs, torch.zeros(N, 34), emb)
        rough = torch.rand(N, 1, generator=torch.Generator().manual_seed(4)) * 1.5
        mid_r = cpu_ref.mid_color(P, fs, cpu_ref.integrated_sh(d, rough), emb)
    want = {"sigma": sig, "raw_density": raw, "embedding": emb, "pred_normals": pn, "n_dot_d": (d * pn).sum(-1), "diff": diff,
            "tint": tint, "roughness": torch.sigmoid(rr), "raw_roughness": rr, "color": diff + tint * mid}
    got = G.gauss_reference(P, fs, m, cd, d, dtype=f32)
    for k in OUTPUTS:
        assert got[k].dtype == f32 and torch.allclose(got[k].reshape(N, -1), want[k].reshape(N, -1), rtol=0, atol=2e-6), k
    nodir = G.gauss_reference(P, fs, m, None, None, dtype=f32)
    assert float(nodir["n_dot_d"].abs().max()) == 0.0
    with torch.no_grad():
        _, emb_u, _ = cpu_ref.density_from_encoding(P, fs, cpu_ref.ipe(fs, m, None))
        d_u, t_u = (torch.sigmoid(cpu_ref.head(P, "field_output_" + h, emb_u)) for h in ("diff", "tint"))
        want_u = d_u + t_u * cpu_ref.mid_color(P, fs, torch.zeros(N, 34), emb_u)
    assert torch.allclose(nodir["color"], want_u, rtol=0, atol=2e-6)
    # embedding mode, on the kernels' padded rows
    W = G.kernel_width(fs.width)
    padded = torch.nn.functional.pad(emb, (0, W - fs.width))
    a = G.emb_reference(P, fs, padded, None, None, True, dtype=f32)  # the head getters
    for k in OUTPUTS:
        ref_k = (diff + tint * low) if k == "color" else (torch.zeros(N) if k == "n_dot_d" else want[k])
        assert torch.allclose(a[k].reshape(N, -1), ref_k.reshape(N, -1), rtol=0, atol=2e-6), k
    b = G.emb_reference(P, fs, padded, d, rough.reshape(N), False, dtype=f32)  # get_mid
    assert torch.allclose(b["color"], mid_r, rtol=0, atol=2e-6)
    c = G.emb_reference(P, fs, padded, None, None, False, dtype=f32)  # get_low
    assert torch.allclose(c["color"], low, rtol=0, atol=2e-6)
    e = G.emb_reference(P, fs, padded, d, None, True, dtype=f32)  # directions without an explicit roughness
    assert torch.allclose(e["color"], want["color"], rtol=0, atol=2e-6) and torch.allclose(e["n_dot_d"], want["n_dot_d"], rtol=0, atol=2e-6)


def test_fp64_reference_is_close_to_float32_and_normals_match_autograd_of_the_chain():
    _, P, fs = G.make_field(4, 128)
    gi = G.gauss_inputs(200, seed=5)
    r64 = G.gauss_reference(P, fs, gi["means"], gi["cov_diag"], gi["view_dirs"])
    r32 = G.gauss_reference(P, fs, gi["means"], gi["cov_diag"], gi["view_dirs"], dtype=f32)
    assert r64["color"].dtype == f64
    for k in ("sigma", "color", "diff", "tint", "roughness", "embedding"):
        assert float((r64[k] - r32[k].double()).abs().max()) <= 1e-4, k
    n, gn = G.gauss_normals_reference(P, fs, gi["means"], gi["cov_diag"], chunk=64)
    with G.default_dtype(f64):
        m = gi["means"].double().requires_grad_(True)
        P64 = {k: v.double() for k, v in P.items()}
        _, _, raw = cpu_ref.density_from_encoding(P64, fs, cpu_ref.ipe(fs, m, gi["cov_diag"].double()))
        (g,) = torch.autograd.grad(raw.sum(), m)
    assert torch.allclose(n, -g / g.norm(dim=-1, keepdim=True), rtol=0, atol=1e-12) and torch.allclose(gn, g.norm(dim=-1))
    assert float((n.norm(dim=-1) - 1).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------- inputs and the exclusion cap
def test_input_builders():
    _, P, fs = G.make_field(8, 200)
    gi = G.gauss_inputs(1000, seed=1)
    assert all(gi[k].dtype == f32 for k in gi) and float(gi["means"].norm(dim=-1).max()) <= 2.0 + 1e-6
    assert float(gi["means"].norm(dim=-1).min()) < 1.0 < float(gi["means"].norm(dim=-1).max())  # both sides of the contraction's branch
    assert 1e-4 * (1 - 1e-6) <= float(gi["cov_diag"].min()) and float(gi["cov_diag"].max()) <= 1e-2 * (1 + 1e-6)
    assert float((gi["view_dirs"].norm(dim=-1) - 1).abs().max()) <= 1e-6
    assert G.gauss_inputs(10, seed=1, damped=False)["cov_diag"] is None
    assert torch.equal(G.gauss_inputs(1000, seed=1)["means"], gi["means"])
    ei = G.emb_inputs(1000, 256, 2, P, fs)
    e = ei["embedding"]
    assert e.shape == (1000, 256) and e.dtype == f32 and float(e.min()) == 0.0 and float(e[:, 200:].abs().max()) == 0.0
    zeros = float((e[:, :200] == 0).float().mean())
    assert 0.2 <= zeros <= 0.8, zeros
    assert 0.0 <= float(ei["roughness"].min()) and float(ei["roughness"].max()) <= 1.5
    for n in (G.n_loop128(G.MI355X_CUS), G.n_loop256(G.MI355X_CUS), G.N_SMALL):
        assert n % 128 and n % 256
    assert G.N_SMALL == 2 * 128 + 77 and 77 == 2 * 32 + 13


_SETS = G.input_sets()


@pytest.mark.parametrize("label,key,kind,N,seed", _SETS, ids=[s[0] for s in _SETS])
def test_exclusion_cap_holds_on_the_reference_alone(label, key, kind, N, seed):
    """Every input set of tests/test_granular_gpu.py (at the MI355X's 256 CUs): at most 0.5 % of the points have an fp64
    |raw normal head| below 1e-2 -- and, for the training case, an fp64 |d raw_density / d mean| below 1e-3 of the median."""
    _, P, fs = G.make_field(*key)
    inp = G.build_inputs(key, kind, N, seed)
    if kind == "emb":
        ref = G.emb_reference(P, fs, inp["embedding"], None, None, True)
    else:
        ref = G.gauss_reference(P, fs, inp["means"], inp["cov_diag"], None)
    hn = ref["normal_head"].norm(dim=-1)
    keep = G.kept_points(label, hn, G.HEAD_MIN)
    print(f"[{label}] |raw normal head| {float(hn.min()):.2e} .. {float(hn.max()):.2e}; {int((~keep).sum())} of {N} points left out")
    if label == "train gauss":
        _, gn = G.gauss_normals_reference(P, fs, inp["means"], inp["cov_diag"])
        keep = G.kept_points(label + " normals", gn, G.GRAD_MIN_REL * float(gn.median()))
        print(f"[{label}] |d raw_density / d mean| median {float(gn.median()):.2e}, min {float(gn.min()):.2e}; {int((~keep).sum())} left out")


# ---------------------------------------------------------------------------------------------- rounded operands
def test_rounded_reference():
    _, P, fs = G.make_field(8, 64)
    gi = G.gauss_inputs(150, seed=6)
    args = (P, fs, gi["means"], gi["cov_diag"], gi["view_dirs"])
    plain = G.gauss_reference(*args)
    same = G.rounded(G.gauss_reference, f64)(*args)
    r16 = G.rounded(G.gauss_reference, torch.bfloat16)(*args)
    again = G.gauss_reference(*args)  # F.linear is put back
    for k in OUTPUTS:
        assert torch.equal(plain[k], same[k]) and torch.equal(plain[k], again[k]), k
        assert r16[k].dtype == f64
    for k, lo, hi in (("color", 1e-5, 3e-2), ("embedding", 1e-5, 3e-2), ("pred_normals", 1e-5, 0.5)):
        e = float((r16[k] - plain[k]).abs().max())
        assert lo < e < hi, (k, e)
    ei = G.emb_inputs(150, 64, 7, P, fs)
    eargs = (P, fs, ei["embedding"], ei["view_dirs"], ei["roughness"], False)
    assert torch.equal(G.rounded(G.emb_reference, f64)(*eargs)["color"], G.emb_reference(*eargs)["color"])
    assert float((G.rounded(G.emb_reference, torch.bfloat16)(*eargs)["color"] - G.emb_reference(*eargs)["color"]).abs().max()) > 1e-6


# ---------------------------------------------------------------------------------------------- geometry
def test_geometry_references():
    """The fp64 contract of a full covariance and the reflection against cpu_ref.contract / F.normalize in float64."""
    inp = FM.build_inputs()
    with G.default_dtype(f64):
        eb = inp["eb"].double()
        mean, cov = cpu_ref.gaussian_blob(inp["o"].double(), inp["d"].double(), inp["pa"].double().reshape(-1, 1), eb[:, :-1], eb[:, 1:])
        mean, cov = mean.reshape(-1, 3), cov.reshape(-1, 3, 3)
        mc, cc = cpu_ref.contract(mean, cov)
    m2, c2 = G.contract(mean, cov)
    assert mean.shape[0] > 256 and mean.shape[0] % 256
    assert torch.allclose(m2, mc, rtol=1e-13, atol=0) and torch.allclose(c2, cc, rtol=1e-9, atol=1e-18 + 1e-12 * float(cc.abs().max()))
    assert float(torch.diagonal(c2, dim1=-2, dim2=-1).min()) >= 0.0
    ri = G.reflection_inputs()
    n = ri["d"].shape[0]
    assert n > 256 and n % 256 and sorted(ri["names"]) == sorted(["unit", "n_is_d", "n_is_minus_d", "n_perp_d", "zero_normal", "dir_half", "dir_two"])
    refl, dot = G.reflection(ri["d"], ri["n"])
    d, nn = ri["d"].double(), ri["n"].double()
    want = torch.nn.functional.normalize(d - 2 * (d * nn).sum(-1, keepdim=True) * nn, dim=-1)
    assert torch.allclose(refl, want, rtol=0, atol=1e-14) and torch.allclose(dot, (d * nn).sum(-1), rtol=0, atol=1e-15)
    z = ri["cls"] == ri["names"].index("zero_normal")
    assert torch.allclose(refl[z], torch.nn.functional.normalize(d[z], dim=-1)) and float(dot[z].abs().max()) == 0.0
    p = ri["cls"] == ri["names"].index("n_is_d")
    assert torch.allclose(refl[p], -d[p], atol=1e-6) and float(dot[ri["cls"] == ri["names"].index("n_perp_d")].abs().max()) < 1e-6


# ---------------------------------------------------------------------------------------------- argument errors, before any launch
@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def _host_args():
    """A valid descriptor and host-side stand-ins for device pointers: every call below returns before it would touch them."""
    f, _, _ = G.make_field(4, 128)
    f.set_mma_mode("f32")
    desc = _abi.FieldDesc.from_buffer_copy(f.field_desc())
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf))
    out = _abi.FieldOutputs()
    out.sigma = p
    saved = _abi.FieldSaved()
    for name in ("enc", "act", "bott", "sh", "hid", "heads", "relu_bits"):
        setattr(saved, name, p)
    return desc, buf, p, out, saved


def test_gaussians_argument_errors(lib):
    desc, buf, p, out, saved = _host_args()
    INVALID, UNSUPPORTED, OK = -1, -2, 0
    fwd, trn = lib.rsn_field_forward_gaussians, lib.rsn_field_forward_gaussians_train
    assert fwd(C.byref(desc), p, -1, p, None, None, C.byref(out), None, None) == INVALID and b"n_points=-1" in lib.rsn_last_error()
    assert fwd(C.byref(desc), p, 5, None, None, None, C.byref(out), None, None) == INVALID and b"means" in lib.rsn_last_error()
    assert fwd(None, p, 5, p, None, None, C.byref(out), None, None) == INVALID
    assert fwd(C.byref(desc), p, 5, p, None, None, None, None, None) == INVALID
    assert fwd(C.byref(desc), p, 0, None, None, None, C.byref(out), None, None) == OK
    assert trn(C.byref(desc), p, -1, p, None, None, C.byref(out), None, C.byref(saved), None) == INVALID
    assert trn(C.byref(desc), p, 5, None, None, None, C.byref(out), None, C.byref(saved), None) == INVALID
    assert trn(None, p, 5, p, None, None, C.byref(out), None, C.byref(saved), None) == INVALID
    assert trn(C.byref(desc), p, 5, p, None, None, None, None, C.byref(saved), None) == INVALID
    assert trn(C.byref(desc), p, 5, p, None, None, C.byref(out), None, None, None) == INVALID
    assert trn(C.byref(desc), p, 0, None, None, None, C.byref(out), None, C.byref(saved), None) == OK
    for mode in (_abi.RSN_MMA_BF16X6, _abi.RSN_MMA_BF16X3, _abi.RSN_MMA_BF16):
        d2 = _abi.FieldDesc.from_buffer_copy(desc)
        d2.mma_mode = mode
        assert trn(C.byref(d2), p, 5, p, None, None, C.byref(out), None, C.byref(saved), None) == UNSUPPORTED, mode
        assert b"exact-fp32" in lib.rsn_last_error()
    assert float(max(buf)) == 0.0 and float(min(buf)) == 0.0  # nothing was written through the stand-in pointer


def test_embedding_argument_errors(lib):
    desc, buf, p, out, _ = _host_args()
    emb = lib.rsn_field_forward_embedding
    assert emb(C.byref(desc), p, -1, p, None, None, C.byref(out), None) == -1 and b"n_points=-1" in lib.rsn_last_error()
    assert emb(C.byref(desc), p, 5, None, None, None, C.byref(out), None) == -1 and b"embedding" in lib.rsn_last_error()
    assert emb(None, p, 5, p, None, None, C.byref(out), None) == -1
    assert emb(C.byref(desc), p, 5, p, None, None, None, None) == -1
    assert emb(C.byref(desc), p, 0, None, None, None, C.byref(out), None) == 0
    assert float(max(buf)) == 0.0 and float(min(buf)) == 0.0


# ---------------------------------------------------------------------------------------------- the rule has to reject these
def _as_kernel(r, W):
    """A reference result shaped like what the GPU file reads back: float32 rows, the embedding padded to the kernel width."""
    out = {k: r[k].float() for k in G.ALL}
    out["embedding"] = torch.nn.functional.pad(r["embedding"].float(), (0, W - r["embedding"].shape[1]))
    return out


def test_rule_accepts_the_float32_oracle_and_rejects_mutations():
    """granular_reference.judge on 333 points in tiles of 128 on a grid of 2 (tile 2 is loop iteration 1): the float32 oracle and
    the rounded-bf16 forward pass; the mistakes the GPU file exists to catch do not."""
    _, P, fs = G.make_field(8, 200)
    N, tile, grid, W = G.N_SMALL, 128, 2, 256
    gi = G.gauss_inputs(N, seed=30)
    m, cd, d = gi["means"], gi["cov_diag"], gi["view_dirs"]
    ref = G.gauss_reference(P, fs, m, cd, d)
    good = _as_kernel(G.gauss_reference(P, fs, m, cd, d, dtype=f32), W)
    G.judge("clean f32", "f32", good, ref, N, tile, grid)
    G.judge("clean bf16x6", "bf16x6", good, ref, N, tile, grid)

    def rejected(label, got, match, reference=ref, mode="f32", r16=None):
        with pytest.raises(AssertionError, match=match):
            G.judge(label, mode, got, reference, N, tile, grid, r16)

    # the second iteration reads or writes its rows one point off (a per-tile address that is right for the first tile only)
    for k in G.ALL + ("embedding",):
        bad = dict(good)
        bad[k] = torch.cat([good[k][:2 * tile], good[k][2 * tile:].roll(1, 0)])
        rejected("shifted second iteration", {k: bad[k]}, "iteration 1")
    # the partly valid wave's 13 rows never written
    bad = dict(good)
    bad["sigma"] = good["sigma"].clone()
    bad["sigma"][N - 13:] = float("nan")
    rejected("unwritten ragged wave", bad, "sigma")
    # padded units that are not exact zeros
    bad = dict(good)
    bad["embedding"] = good["embedding"].clone()
    bad["embedding"][5, 201] = 1e-30
    rejected("padding", bad, "padded embedding columns")
    # flags ignored: the covariance, the directions
    rejected("undamped where damped", _as_kernel(G.gauss_reference(P, fs, m, None, d, dtype=f32), W), "sigma")
    nodir = G.gauss_reference(P, fs, m, cd, None)
    rejected("SH inputs not zeroed", {"color": good["color"]}, "color", reference=nodir)
    rejected("n_dot_d without directions", {"n_dot_d": good["n_dot_d"]}, "n_dot_d", reference=nodir)
    # embedding mode: the explicit roughness ignored, the colour combine of the wrong branch
    ei = G.emb_inputs(N, W, 40, P, fs)
    e, dd, rg = ei["embedding"], ei["view_dirs"], ei["roughness"]
    mid = G.emb_reference(P, fs, e, dd, rg, False)
    G.judge("clean get_mid", "f32", {"color": G.emb_reference(P, fs, e, dd, rg, False, dtype=f32)["color"].float()}, mid, N, tile, grid)
    rejected("rho from the head", {"color": G.emb_reference(P, fs, e, dd, None, False, dtype=f32)["color"].float()}, "color", reference=mid)
    rejected("diff + tint * mid where mid alone", {"color": G.emb_reference(P, fs, e, dd, rg, True, dtype=f32)["color"].float()}, "color",
             reference=mid)
    # plain bf16: the rounded forward itself passes, a unit vector from the neighbouring point does not
    r16 = G.rounded(G.gauss_reference, torch.bfloat16)(P, fs, m, cd, d)
    g16 = _as_kernel(r16, W)
    G.judge("clean bf16", "bf16", g16, ref, N, tile, grid, r16)
    rejected("bf16 shifted normals", {"pred_normals": g16["pred_normals"].roll(1, 0)}, "pred_normals", mode="bf16", r16=r16)
    # the float32 oracle against itself under the fp32 rule of the undamped case, and a 1e-3 slip that rule has to see
    ru, ou = G.gauss_reference(P, fs, m, None, d), G.gauss_reference(P, fs, m, None, d, dtype=f32)
    gu = _as_kernel(ou, W)
    G.judge_against_oracle("clean undamped", gu, ru, ou, N)
    G.judge("clean undamped against the oracle", "f32", gu, ou, N, tile, grid)
    with pytest.raises(AssertionError):
        G.judge("undamped slip", "f32", {"color": gu["color"] + 3e-4}, ou, N, tile, grid)
