"""The derivative GEMMs of the exact-fp32 training kernels on SIX of the nine piece products (rsn_gemm_loops.h, NP = 6): the loop
GEMMs of the analytic-normal sweep of rsn_field_kernel<NB, true, 0 | 4>, and the weight gradients of an exact-fp32 step on the
split-bf16 reduction.  The dropped products are w_lo b_lo, w_lo b_mid and w_mid b_lo.  Stage 4 of rsn_field_bwd_kernel<NB, 4> was
measured on six and stays on nine; the cases here hold for either count and judge it as it is.

The integer cases of tests/test_normals_x9_gpu.py and tests/test_backward_x9_gpu.py hold weights of -2 .. 2, whose mid and lo pieces
are zero: they cannot tell which count runs.  Here:

  1. kept products present and in place.  The trunk layer under the top one holds integers of up to 19 bits (with nearest-rounding
     pieces a 17-bit integer has no lo piece: hi, mid and lo are all non-zero from 2^18 on, which is asserted), one or two a column;
     the top trunk layer and every trunk layer below the wide one are signed permutations; the density row is +-1.  The operand
     that meets the wide weights is then 0 / +-1 in the normal sweep (a small integer, hi piece only, in the backward sweep),
     so w_mid b_hi and w_lo b_hi carry the sum; the wide result then meets the permutation below it (L4skip) and, in the normal sweep,
     the raw-coordinate integers of the encoded-input part, where w_hi b_mid and w_hi b_lo carry it.  Every dropped product has a zero
     factor and every partial sum is an integer below 2^24 (asserted), so normals equal the fp64 direction to 1e-6 (the normalisation
     alone) and every dy row equals the host's integer sums bit for bit.  A missing or misplaced kept product gives another integer.
  2. random fp32 fields (all three pieces on both sides) at widths 32, 64, 256 and 16, 17, 31, 32, 49 points: normals and every
     dy[l] under field_maths_reference.compare's rule (4 x the float32 restatement's error + 1 ulp); folded and unfolded normals
     bit-equal.
  3. on those cases act, relu_bits, sigma, heads and hid of the training forward equal a forward launched without the sweep.
  4. the weight gradients of an exact-fp32 field through _weight_grads equal the same call with the mode forced to RSN_MMA_BF16X6
     bit for bit (ordered flush); EVERY parameter gradient lies within 2e-5 max|ref| of the fp64 products of the saved rows (the
     column maps of the encoded / SH inputs and, folded, the unfold formula restated in fp64); _WGRAD_MODE is still 0, and a bare
     _wgrad_multi is still the fp32 reduction, whose bits differ from the split-bf16 one's.
  5. two deterministic steps of a 4 x 64 field on 64 rays are bit-equal.
No constant here comes from a run of the kernels."""
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, train_graph
from tests import field_maths_reference as R
from tests import layer_gemm_reference as G
from tests import test_backward_x9_gpu as BX
from tests import test_deterministic_gpu as DT
from tests import test_layer_gemms_gpu as LG
from tests import test_multitile_gpu as MT
from tests import test_normals_seed_gpu as S
from tests import test_normals_x9_gpu as X9

pytestmark = pytest.mark.gpu

INT_NETS = {"L3": (3, ()), "L4skip": (4, (2,))}
WIDTHS = (32, 64, 256)
RAW_ROWS = 4  # rows of an encoded-input part that read the raw coordinates


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- 1. kept products
def _widen(f, width, layers, skips, per_column):
    """Overwrites the trunk x parts of an integer field: layer L-2 wide (|w| < 2^19, per_column a column and a row), every other
    layer l >= 1 a signed permutation; the raw-coordinate integers of the encoded-input parts stay on RAW_ROWS rows, which layer 0
    keeps live, and the biases of the layers above fix their masks (the same at every point: what is tested here is which products
    meet which, the masks have tests/test_normals_shape16_gpu.py); the density row becomes +-1.  Bound on the normal sweep's
    partial sums (per_column = 2): the operand of the wide GEMM is at most 1, its result below 2 * 2^19 = 2^20, a permutation keeps
    that, and an encoded-input GEMM multiplies by at most 2 * RAW_ROWS = 8: 2^23 * 1.01^2 < 2^24 (pieces of an integer are integers whose magnitudes sum to less than 1.01 times the
    value's).  The backward sweep's operand is a small integer, not 0 / +-1: per_column = 1 there, and the test asserts the bound."""
    i, j = torch.arange(width)[:, None], torch.arange(width)[None, :]
    raw = (torch.arange(width) % (width // RAW_ROWS)) == 1
    with torch.no_grad():
        for l in range(layers):
            lin = f.mlp_base.layers[l]
            w = lin.weight.clone()
            in_f = w.shape[1]
            if l == 0 or l in skips:
                w[~raw, 96:99] = 0.0
            if l == layers - 2 and l >= 1:
                wide = ((i * 40503 + j * 9973 + 12345) % 1048575 - 524287) * (((i - 3 * j) % width) < per_column)
                w[:, in_f - width:] = wide.float()
            elif l >= 1:
                w[:, in_f - width:] = (((i % 2) * 2 - 1) * (j == (5 * i + 1) % width)).float()
            lin.weight.copy_(w)
        f.mlp_base.layers[0].bias[raw] = 50.0
        # masks of the layers l >= 1 fixed by the biases, two units in three live: a pre-activation stays below 60 under the wide
        # layer, 2 * 2^19 * 1e4 in it and 1e13 + 1e11 above it, so a bias of +-B_l decides the sign at every point
        for l in range(1, layers):
            big = 1e4 if l < layers - 2 else (1e13 if l == layers - 2 else 1e17)
            f.mlp_base.layers[l].bias.copy_(torch.where((torch.arange(width) + l) % 3 != 0, big, -big))
        f.field_output_density.net.weight.copy_((((torch.arange(width) // 2) % 2) * 2.0 - 1.0).reshape(1, width))
    wl = f.mlp_base.layers[layers - 2].weight[:, -width:].detach()
    for t in (wl, wl - wl.bfloat16().float(), wl - wl.bfloat16().float() - (wl - wl.bfloat16().float()).bfloat16().float()):
        assert float(t.abs().max()) > 0, "the wide layer lacks one of its three pieces"
    return f


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("net", list(INT_NETS))
def test_kept_products_normal_sweep(dev, width, net):
    layers, skips = INT_NETS[net]
    f = _widen(X9._integer_field(width, layers, skips), width, layers, skips, 2)
    inp = S._rays(37, 3, seed=width + layers)
    res = {}
    for fold in (False, True):
        got, act, means = S._run(dev, f, inp, fold)
        ref, ora = S._references(f, layers, X9._skip(skips), inp, act, means)
        # the host's sweep in integers: every partial sum in the exact range
        P = {k: v.detach().cpu().double() for k, v in f.state_dict().items()}
        g = P["field_output_density.net.weight"].abs().expand(act.shape[1], width)
        for l in range(layers - 1, 0, -1):
            g = g @ P[f"mlp_base.layers.{l}.weight"][:, -width:].abs()
        assert float((g @ P["mlp_base.layers.0.weight"][:, 96:99].abs()).max()) * 1.01 ** 2 < 2.0 ** 24
        live = float((ref.norm(dim=-1) > 0.5).float().mean())
        err = float((got.double() - ref).abs().max())
        print(f"[w{width} {net} fold={fold}] wide integers: worst |normals - fp64| {err:.3e}, {live:.2f} of the points carry a gradient "
              f"(the float32 sweep: {float((ora.double() - ref).abs().max()):.3e})")
        assert live > 0.25, "too few points carry a gradient through the wide layer: the case tells nothing"
        assert err <= 1e-6
        res[fold] = got
    assert torch.equal(res[False], res[True]), "folded and unfolded normals differ"


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("net", list(INT_NETS))
def test_kept_products_backward_stage4(dev, width, net):
    layers, skips = INT_NETS[net]
    skip = skips[0] if skips else -1
    f = _widen(BX._integer_net(width, layers, skips), width, layers, skips, 1)
    f.to(dev).train()
    f.set_mma_mode("f32")
    inp = S._rays(BX.M_INF, 2, seed=width + layers)
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    sq, d_inf = inf["sq"][:BX.M_INF].contiguous(), inf["d"][:BX.M_INF].contiguous()
    g_bg = 4.0 * torch.randint(-1, 2, (BX.M_INF, 3), generator=torch.Generator().manual_seed(width + layers)).float()
    P = BX._host(f.state_dict())
    for fold in (True, False):
        saved = BX._inf_forward(dev, f, inp, d_inf, sq, fold)
        act = saved["act"].cpu()
        go = BX._inf_backward(dev, f, d_inf, sq, saved, g_bg, False, fold)
        dy = go["dy"].reshape(layers, BX.M_INF, -1)
        assert bool(torch.isfinite(dy).all()) and bool((dy == dy.round()).all()), "the layer gradients are not integers"
        assert float(dy[layers - 1].abs().max()) > 0, "no gradient reaches the trunk: the case tells nothing"
        for l in range(layers - 1, 0, -1):
            w = P[f"mlp_base.layers.{l}.weight"].double()
            w = w[:, 99:] if l == skip else w
            x = dy[l][:, :width].double()
            assert float((x.abs() @ w.abs()).max()) * 1.01 ** 2 < 2.0 ** 24, "a partial sum may leave the exact range: not an exact case"
            want = (x @ w) * (act[l - 1][:, :width] > 0)
            assert torch.equal(dy[l - 1][:, :width].double(), want), f"fold={fold}: dy[{l - 1}] differs from the host's integer sums"
            assert bool((dy[l - 1][:, width:] == 0).all())
        assert float(dy[max(layers - 3, 0)].abs().max()) >= 256, "no wide value left the wide GEMM: the case tells nothing"


# ---------------------------------------------------------------------------------------------- 2 and 3. random fields
POINTS = {"16": (16, 1), "17": (17, 1), "31": (31, 1), "32": (32, 1), "49": (49, 1)}
_FWD_KEYS = ("sigma", "raw_density", "color", "pred_normals", "n_dot_d", "diff", "tint", "roughness")
_SAVED_KEYS = ("act", "relu_bits", "heads", "hid", "enc", "sh")


@pytest.mark.parametrize("points", list(POINTS))
@pytest.mark.parametrize("width", WIDTHS)
def test_random_fields_normals_and_sign_decisions(dev, width, points):
    Rn, Sn = POINTS[points]
    f, inp = S._field(width), S._rays(Rn, Sn, seed=width + Rn)
    res = {fold: S._run(dev, f, inp, fold) for fold in (False, True)}
    (n0, act0, m0), (n1, act1, m1) = res[False], res[True]
    assert bool(torch.isfinite(n0).all()) and torch.equal(act0, act1) and torch.equal(m0, m1)
    assert torch.equal(n0, n1), "folded and unfolded normals differ"
    ref, ora = S._references(f, 8, 4, inp, act0, m0)
    S._judge(f"w{width} {points} points", n0, ref, ora)
    # 3. what the sweep must not touch: the same forward with and without it
    rays = tuple(inp[k].to(dev) for k in ("o", "d", "pa", "eb"))
    for fold in (False, True):
        with LG._launching(), LG._poisoned_allocators(f):
            a = f.evaluate_frustums_train(*rays, want_normals=True, fold=fold)
            b = f.evaluate_frustums_train(*rays, want_normals=False, fold=fold)
        for k in _FWD_KEYS:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"fold={fold}: {k} differs with the normal sweep on"
        for k in _SAVED_KEYS:
            assert torch.equal(a["saved"][k].view(torch.int32), b["saved"][k].view(torch.int32)), f"fold={fold}: saved {k} differs with the normal sweep on"


@pytest.mark.parametrize("points", list(POINTS))
@pytest.mark.parametrize("width", WIDTHS)
def test_random_fields_layer_gradients(dev, width, points):
    layers, skips = LG.NETS["L8"]
    Rn, Sn = POINTS[points]
    n = Rn * Sn
    f = S._field(width, layers=layers, skips=skips, seed=23)
    inp = S._rays(Rn, Sn, seed=width + layers + Rn)
    f.to(dev).train()
    f.set_mma_mode("f32")
    lay, ring = LG._kernel(f, "f32", width)
    rays = (inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev))
    eb = inp["eb"].to(dev)
    gin = LG._gin(Rn, Sn, Rn + width, dev)
    with LG._launching(), LG._poisoned_allocators(f):
        lv = f.evaluate_frustums_train(*rays, eb, want_normals=True, fold=True)
        go = train_graph._field_backward(f, rays, eb, lv, gin, True, fold=True)
    rows = LG._rows(n, lv, lv["saved"], go, True)
    P = BX._host(f.state_dict())
    r64 = G.restate(P, lay, rows, layers, skips[0], "f32", True, ring)
    r32 = G.restate(P, lay, rows, layers, skips[0], "f32", True, ring, dtype=torch.float32)
    bad = []
    for l in range(layers - 1):
        key = f"dy[{l}]"
        v = R.compare(f"w{width} {points} points", key, r64[key].got.double(), r64[key].ref, r32[key].ref.double(),
                      torch.zeros(n, dtype=torch.long), ["all"])
        print(v.report())
        if not v.ok:
            bad.append(v.report())
    assert not bad, "\n" + "\n".join(bad)


# ---------------------------------------------------------------------------------------------- 4. weight gradients
def _fp64_weight_grads(f, saved, go, fold):
    """Every parameter gradient _weight_grads produces for one frustum level with heads, in fp64 from the saved rows: dW = dY^T X and
    db = column sums of dY per linear layer, the encoded / SH inputs brought from slot order to the reference's columns by the
    layout's maps; with `fold`, the bottleneck's and mlp_mid's x-part gradients by rsn_unfold_bottleneck_grads' formula
    (include/rsn.h) on c = d a_mid^T act[L-1] and s = the column sums of d a_mid."""
    L, W = f.mlp_base.num_layers, f.param_width
    skip = f.field_desc().skip_layer
    lay = f.train_layout()
    h = lambda t: t.detach().double().cpu()  # noqa: E731
    P = {k: h(v) for k, v in f.state_dict().items()}
    enc = G.columns(saved["enc"].detach().cpu(), lay["enc_map"], 99, torch.float64)
    sh = G.columns(saved["sh"].detach().cpu(), lay["sh_map"], 34, torch.float64)
    act, hid, dy = h(saved["act"])[:, :, :W], h(saved["hid"]), h(go["dy"])[:, :, :W]
    da, dzr, dzh = h(go["da_mid"]), h(go["dz_rgb"])[:, :3], h(go["dz_heads"])
    emb = act[L - 1]
    ref = {}
    for l in range(L):
        if l == 0:
            x = enc
        elif l == skip:
            x = torch.cat([enc, act[l - 1]], dim=1)  # encoded inputs first (nerfstudio's MLP)
        else:
            x = act[l - 1]
        ref[f"mlp_base.layers.{l}.weight"], ref[f"mlp_base.layers.{l}.bias"] = dy[l].t() @ x, dy[l].sum(0)
    if fold:
        c, s = da.t() @ emb, da.sum(0)
        w_mx, w_b, b_b = P["mlp_mid.layers.0.weight"][:, 34:34 + W], P["field_output_bottleneck.net.weight"], P["field_output_bottleneck.net.bias"]
        mid_x = c @ w_b.t() + s[:, None] * b_b[None, :]
        ref["field_output_bottleneck.net.weight"], ref["field_output_bottleneck.net.bias"] = w_mx.t() @ c, w_mx.t() @ s
    else:
        d_bott = h(go["d_bott"])[:, :W]
        mid_x = da.t() @ h(saved["bott"])[:, :W]
        ref["field_output_bottleneck.net.weight"], ref["field_output_bottleneck.net.bias"] = d_bott.t() @ emb, d_bott.sum(0)
    ref["mlp_mid.layers.0.weight"], ref["mlp_mid.layers.0.bias"] = torch.cat([da.t() @ sh, mid_x], dim=1), da.sum(0)
    ref["field_output_mid.net.weight"], ref["field_output_mid.net.bias"] = dzr.t() @ hid, dzr.sum(0)
    # rows of the 16-row heads block (train_graph._GradAcc.finish)
    for name, lo, hi in (("density", 0, 1), ("normals", 1, 4), ("diff", 4, 7), ("roughness", 8, 9), ("tint", 12, 15)):
        ref[f"field_output_{name}.net.weight"], ref[f"field_output_{name}.net.bias"] = dzh[:, lo:hi].t() @ emb, dzh[:, lo:hi].sum(0)
    return ref


@pytest.mark.parametrize("layers,width", [(8, 256), (2, 64)])
@pytest.mark.parametrize("fold", [False, True], ids=["plain", "fold"])
def test_weight_grads_of_an_exact_field_run_the_split_reduction(dev, layers, width, fold):
    f = MT._one_job_field(dev, "f32", layers, width)
    job, _, _ = MT._one_job_inputs(0, dev)
    o, d, pa, eb = job["rays"]
    lv = f.evaluate_frustums_train(o, d, pa, eb, want_normals=True, fold=fold)
    go = train_graph._field_backward(f, (o, d, pa), eb, lv, job["gin"], True, fold=fold)

    def grads(mode):
        acc = train_graph._GradAcc(f)
        real = f.mma_mode
        try:
            if mode is not None:
                f.mma_mode = mode
            train_graph._weight_grads(f, [(lv["saved"], go, True)], acc, ordered=True, fold=fold)
        finally:
            f.mma_mode = real
        return {k: v.clone() for k, v in acc.finish().items()}

    own, forced = grads(None), grads(_abi.RSN_MMA_BF16X6)
    assert train_graph._WGRAD_MODE == 0 and train_graph._WGRAD_ORDERED is False
    assert int(f.mma_mode) == _abi.RSN_MMA_F32
    for k in own:
        assert bool(torch.isfinite(own[k]).all()), k
        assert torch.equal(own[k], forced[k]), f"{k}: the exact-fp32 field's weight gradient is not the split-bf16 reduction's"
    # every parameter gradient against the fp64 products of the saved rows
    ref = _fp64_weight_grads(f, lv["saved"], go, fold)
    assert set(own) == set(ref), sorted(set(own) ^ set(ref))
    for k in sorted(own):
        got, want = own[k].double().cpu(), ref[k]
        assert got.shape == want.shape, k
        err, bound = float((got - want).abs().max()), 2e-5 * float(want.abs().max())
        print(f"{layers} x {width} fold={fold} {k}: err {err:.3e} / bound {bound:.3e}")
        assert float(want.abs().max()) > 0, f"{k}: the reference gradient is zero: the case tells nothing"
        assert err <= bound, k
    # a bare call is still the fp32 reduction: the bits of a call that names RSN_MMA_F32, within the bound of the fp64 product
    g = torch.Generator().manual_seed(64)
    a, x = torch.randn(300, 64, generator=g), torch.randn(300, 64, generator=g)
    ref = a.double().t() @ x.double()
    out = []
    for mode in (None, _abi.RSN_MMA_F32, _abi.RSN_MMA_BF16X6):
        dw = torch.zeros(64, 64, device=dev)
        train_graph._wgrad_multi([(a.to(dev), x.to(dev))], 64, 64, dw, 0, None, mode=mode, ordered=True)
        out.append(dw.cpu())
        assert float((dw.double().cpu() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    assert torch.equal(out[0], out[1]), "a bare _wgrad_multi is not the fp32 reduction"
    # ... and the two kernels are told apart by their bits here (4,096 sums of 300 products in another order and arithmetic: were
    # all three calls one kernel, the line above would say nothing)
    assert not torch.equal(out[1], out[2]), "RSN_MMA_F32 and RSN_MMA_BF16X6 gave the same bits: the modes cannot be told apart"


# ---------------------------------------------------------------------------------------------- 5. repeatability
def test_two_deterministic_steps_are_bit_equal(dev):
    DT._assert_same_bits(DT._run_steps(dev, 64, 4, 64, "f32", True, 2), DT._run_steps(dev, 64, 4, 64, "f32", True, 2))
