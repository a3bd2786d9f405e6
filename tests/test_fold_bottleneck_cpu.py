"""The folded bottleneck (RSN_MMA_F32_FOLDED) without a GPU: what the library refuses before any launch, the size of the folded
packed buffer, and the algebra the kernels rest on -- the folded forward value and the recovered parameter gradients against fp64
autograd through oracle/cpu_ref.mid_color on the host."""
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi
from reflect_sampling_nerf_amd._build import build_library


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def _desc(width, param_width=0, mode=_abi.RSN_MMA_F32, layers=8, skip=4):
    d = _abi.FieldDesc()
    d.num_layers, d.width, d.skip_layer, d.mid_width, d.density_bias, d.mma_mode, d.param_width = layers, width, skip, 128, 0.5, mode, \
        param_width
    return d


@pytest.mark.parametrize("width,param_width", [(256, 0), (256, 200), (128, 0), (64, 0)])
def test_folded_packed_buffer_is_the_f32_buffer_plus_the_folded_segments(lib, width, param_width):
    """The packed buffer of RSN_MMA_F32 keeps its size; RSN_MMA_F32_FOLDED appends the dense W_c [128, param width] (padded to
    four floats) and b_c [128], the forward segment [W_c ; heads] (K = W in W/8 K-iterations of 5 row blocks) with its 160
    biases, and the transposed segment (20 K-iterations of W/32 row blocks); a mode past it is refused."""
    plain = lib.rsn_packed_weights_bytes(C.byref(_desc(width, param_width)))
    folded = lib.rsn_packed_weights_bytes(C.byref(_desc(width, param_width, _abi.RSN_MMA_F32_FOLDED)))
    pw, nb = (param_width or width), width // 32
    extra = (128 * pw + 3) // 4 * 4 + 128 + (nb * 4) * 5 * 256 + 160 + 20 * nb * 256
    assert plain > 0 and folded == plain + 4 * extra
    assert lib.rsn_packed_weights_bytes(C.byref(_desc(width, param_width, _abi.RSN_MMA_F32_FOLDED + 1))) == 0
    assert b"mma_mode=5" in lib.rsn_last_error()


def test_folded_mode_keeps_the_saved_layout_of_f32(lib):
    def layout(mode):
        d = _desc(256, 0, mode)
        enc_cols, sh_cols, narrow = C.c_int32(), C.c_int32(), C.c_int32()
        enc_map, sh_map = (C.c_int32 * 128)(), (C.c_int32 * 64)()
        assert lib.rsn_train_saved_layout(C.byref(d), C.byref(enc_cols), C.byref(sh_cols), C.byref(narrow), enc_map, sh_map) == 0
        return enc_cols.value, sh_cols.value, narrow.value, list(enc_map), list(sh_map)

    assert layout(_abi.RSN_MMA_F32_FOLDED) == layout(_abi.RSN_MMA_F32)


def test_unfold_entry_point_refuses_bad_sizes_and_null_pointers(lib):
    """rsn_unfold_bottleneck_grads checks its arguments before it launches anything (no GPU here: the pointers are never read)."""
    p = C.c_void_p(4096)  # stands for a device pointer
    ok = dict(width=256, n_mid=128, c=p, ld_c=256, s=p, mid_w=p, ld_mid=290, bott_w=p, bott_b=p, d_bott_w=p, d_bott_b=p, d_mid_w=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.rsn_unfold_bottleneck_grads(a["width"], a["n_mid"], a["c"], a["ld_c"], a["s"], a["mid_w"], a["ld_mid"], a["bott_w"],
                                               a["bott_b"], a["d_bott_w"], a["d_bott_b"], a["d_mid_w"], None)

    for kw, msg in ((dict(width=0), b"width=0"), (dict(width=257), b"width=257"), (dict(n_mid=0), b"n_mid=0"),
                    (dict(ld_c=255), b"ld_c=255"), (dict(ld_mid=289), b"ld_mid=289")):
        assert call(**kw) == -1, kw
        assert msg in lib.rsn_last_error(), (kw, lib.rsn_last_error())
    for name in ("c", "s", "mid_w", "bott_w", "bott_b", "d_bott_w", "d_bott_b", "d_mid_w"):
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.rsn_last_error()


def test_field_folds_only_in_exact_fp32():
    f = pkg.ReflectSamplingNeRFNerfField()
    assert f.folds() and f.field_desc(True).mma_mode == _abi.RSN_MMA_F32_FOLDED and f.field_desc().mma_mode == _abi.RSN_MMA_F32
    assert f.field_desc(True).width == f.field_desc().width and list(f.field_desc(True).freqs) == list(f.field_desc().freqs)
    f.set_mma_mode("bf16x6")
    assert not f.folds()
    with pytest.raises(_abi.RsnError):
        f.field_desc(True)


@pytest.mark.parametrize("width,scale", [(256, 1.0), (200, 1.0), (64, 8.0)])
def test_fold_formulas_against_fp64_autograd_through_the_oracle(width, scale):
    """W_c = W_mx W_b, b_c = b_mid + W_mx b_b give mid_color's value; with C = sum d a_mid (x) a and s = sum d a_mid,
    dW_b = W_mx^T C, db_b = W_mx^T s and dW_mx = C W_b^T + s (x) b_b are the gradients autograd takes through the two layers
    (oracle/cpu_ref.mid_color, fp64, nn.Linear-style parameters at `scale` x).  Pure algebra: 1e-11 of the largest entry.  With
    W_c and b_c rounded to fp32 as rsn_fold_kernel leaves them, every hidden pre-activation moves by at most one rounding (2^-24) of
    each folded entry it sums: 2^-24 (|a| |W_c|^T + |b_c|)."""
    fs = cpu_ref.FieldSpec(num_layers=8, width=width)
    torch.manual_seed(width)
    P = {k: (v.double() * scale).requires_grad_(True) for k, v in cpu_ref.init_params(fs).items()}
    g = torch.Generator().manual_seed(1)
    n = 1280
    emb = torch.relu(torch.randn(n, width, generator=g, dtype=torch.float64))
    sh = torch.randn(n, 34, generator=g, dtype=torch.float64) * 0.3
    up = torch.randn(n, 3, generator=g, dtype=torch.float64)
    (up * cpu_ref.mid_color(P, fs, sh, emb)).sum().backward()
    wm, bm = P["mlp_mid.layers.0.weight"].detach(), P["mlp_mid.layers.0.bias"].detach()
    wb, bb = P["field_output_bottleneck.net.weight"].detach(), P["field_output_bottleneck.net.bias"].detach()
    wmx = wm[:, 34:]
    wc, bc = wmx @ wb, bm + wmx @ bb
    z = (sh @ wm[:, :34].t() + emb @ wc.t() + bc).requires_grad_(True)
    rgb = torch.sigmoid(cpu_ref.head({k: v.detach() for k, v in P.items()}, "field_output_mid", torch.relu(z)))
    ref_rgb = cpu_ref.mid_color({k: v.detach() for k, v in P.items()}, fs, sh, emb)
    assert float((rgb.detach() - ref_rgb).abs().max()) <= 1e-11
    (up * rgb).sum().backward()
    da = z.grad
    c, s = da.t() @ emb, da.sum(0)
    got = {"dW_b": wmx.t() @ c, "db_b": wmx.t() @ s, "dW_mx": c @ wb.t() + s[:, None] * bb[None, :]}
    ref = {"dW_b": P["field_output_bottleneck.net.weight"].grad, "db_b": P["field_output_bottleneck.net.bias"].grad,
           "dW_mx": P["mlp_mid.layers.0.weight"].grad[:, 34:]}
    for k in got:
        err, top = float((got[k] - ref[k]).abs().max()), float(ref[k].abs().max())
        assert top > 0 and err <= 1e-11 * top, (k, err, top)
    # the SH columns and the bias of mlp_mid take d a_mid directly, folded or not
    assert float((da.t() @ sh - P["mlp_mid.layers.0.weight"].grad[:, :34]).abs().max()) <= 1e-11 * float(c.abs().max())
    assert float((s - P["mlp_mid.layers.0.bias"].grad).abs().max()) <= 1e-11 * float(s.abs().max())
    # fp32 storage of the folded weights: one rounding of each entry
    z32 = sh @ wm[:, :34].t() + emb @ wc.float().double().t() + bc.float().double()
    room = 2.0 ** -24 * (emb.abs() @ wc.abs().t() + bc.abs()) + 1e-12
    assert bool(((z32 - z.detach()).abs() <= room).all())
