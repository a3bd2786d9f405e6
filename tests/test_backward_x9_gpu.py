"""Stage 4 of the folded backward sweep on the nine-product loop of the 16x16x32 bf16 MFMA shape (rsn_field_bwd.hip,
rsn_field_bwd_kernel<NB, 4>: gemm_bf16_s16 over the packed pieces hT_last and hT_x[1 .. L-2], its row saver sv_put16,
store_masked_bits16).  Folded mode only.  tests/test_layer_gemms_gpu.py, test_fold_bottleneck_gpu.py, test_gpu_parity.py and
test_multitile_gpu.py judge the sweep as they judged the fp32 loop; here is what the new lane mapping and the new store path can
get wrong at shapes theirs do not reach.

The two encoded-input GEMMs behind the trunk stay on the fp32 loop.  On the nine-product loop (gemm_bf16_s16<4>, store_act16<4>)
every dy record and every bit-for-bit case here passed, but d_input missed field_maths_reference.compare's rule (4 x the float32
oracle's error + 1 ulp) twice on an MI355X: tests/test_layer_gemms_gpu.py f32-fold-w32-L8-1, 1.512e-06 against a bound of
1.004e-06 (oracle 1.572e-07), and test_no_stray_stores[64-300-129-input] below, 2.900e-05 against 2.395e-05 (oracle 4.330e-06);
with them on the fp32 loop both pass, as does every other case of the two files.

Every comparison is against the fp64 restatement and the per-entry bound K u S of tests/layer_gemm_reference.py (imported), on the
kernel's own input rows, unless stated: the integer cases are bit for bit against the host's integer sums, the multi-job and
repeatability cases bit for bit against another launch.  No constant here comes from a run of the kernels.

  1. point halves: 16, 17, 31, 32 and 49 points (the second point half of a wave's tile empty, with one row, lacking one row,
     full, and a second wave that starts in a half), 1, 33 and 300 points; widths 256, 128, 64 and parameter width 200 (padded
     units); nets L2 (only the relocated layer L-1: hT_last), L3 and L8 with its skip; with and without the input gradient (without
     it dy[0] leaves through the tail loop, with it through the saver of the fp32 encoded-input GEMM, both in the standard layout
     behind a 16-shape epilogue).
  2. integer weights and integer upstream gradients through get_inf_color's job (its mid colour set to 1/2, so dz_rgb = g / 4 is
     an integer): every sum of the sweep is exact in fp32 in any order, so every dy[l - 1] equals the host's integer
     mask (dy[l] W_l), and d_input -- exact integer sums g_enc, then the float32 variance chain, which this pull request does not
     touch -- equals the unfolded instantiation's (the fp32 MFMA loop on the same integers) bit for bit.  The live units of each
     masked layer in turn are confined to one 4-row group of every 32-row block, for each of the eight groups (the construction of
     tests/test_normals_shape16_gpu.py): a slip in a row half, nibble or K map gives another integer.
  3. no stray stores: all gradient buffers poisoned, a device-side count below the buffers' size so that the last live wave holds
     1, 16, 17 or 31 rows and whole tiles lie behind it: every live row passes the fp64 rule (so it was written and is finite),
     every row behind the count still holds the poison.
  4. a multi-job launch (two levels of 45 x 3 and 45 x 2 points and get_inf_color: the second job starts inside the 128-point tile
     the first ends in, were the tiles shared) equals the separate launches bit for bit.
  5. two runs of one case are bit-equal."""
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import ops, train_graph
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import field_maths_reference as R
from tests import layer_gemm_reference as G
from tests import test_layer_gemms_gpu as LG
from tests import test_normals_seed_gpu as S
from tests.helpers import _POISON, _poisoned
from tests.test_normals_x9_gpu import _integer_field

pytestmark = pytest.mark.gpu

POINTS = {"1": (1, 1), "16": (16, 1), "17": (17, 1), "31": (31, 1), "32": (32, 1), "33": (11, 3), "49": (49, 1), "300": (100, 3)}
WIDTHS = (256, 128, 64, 200)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


def _host(d):
    return {k: v.detach().cpu() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------- 1. point halves
def _halves_cases():
    c = [(w, "L8", p, True) for w in WIDTHS for p in POINTS]
    c += [(w, n, p, True) for w in (256, 64) for n in ("L2", "L3") for p in ("17", "49")]
    c += [(w, n, "49", False) for w in WIDTHS for n in ("L2", "L3", "L8")]
    c += [(256, "L8", p, False) for p in POINTS if p != "49"]
    return c


def run_without_input_grad(dev, width, net, points, n_live_rays=None):
    """LG.run_case with need_input off: every record of the job but d_input, which does not exist; -> (failures, gout on the host)."""
    layers, skips = LG.NETS[net]
    Rn, Sn = points
    f = S._field(width, layers=layers, skips=skips, seed=23)
    inp = S._rays(Rn, Sn, seed=width + layers + Rn)
    f.to(dev).train()
    f.set_mma_mode("f32")
    lay, ring = LG._kernel(f, "f32", width)
    rays = (inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev))
    eb = inp["eb"].to(dev)
    gin = LG._gin(Rn, Sn, Rn + width, dev)
    n_dev = None if n_live_rays is None else torch.tensor([n_live_rays], dtype=torch.int32, device=dev)
    with LG._launching(), LG._poisoned_allocators(f):
        lv = f.evaluate_frustums_train(*rays, eb, n_dev=n_dev, want_normals=True, fold=True)
        go = train_graph._field_backward(f, rays, eb, lv, gin, False, n_dev=n_dev, fold=True)
    assert "d_input" not in go
    n = Rn * Sn
    live = n if n_live_rays is None else n_live_rays * Sn
    rows = LG._rows(n, lv, lv["saved"], dict(go, d_input=torch.zeros(n)), True)
    del rows["d_input"]
    label = f"f32 folded w{width} {net} {n} points ({live} live), no input gradient"
    for k, t in rows.items():
        lead = t[:, live:] if k in ("act", "dy") else t[live:]
        if lead.numel():
            it, pattern = _POISON[lead.dtype]
            assert bool((lead.contiguous().view(it) == pattern).all()), f"{label} {k}: rows behind the device-side count were written"
    cut = {k: (t[:, :live] if k in ("act", "dy") else t[:live]) for k, t in rows.items()}
    P = _host(f.state_dict())
    recs = G.restate(P, lay, cut, layers, skips[0] if skips else -1, "f32", True, ring)
    assert {f"dy[{l}]" for l in range(layers)} | {"da_mid"} <= set(recs)
    shares, failures = G.judge(label, "f32", recs, ring)
    print(G.report(label, shares))
    return failures, _host(go)


@pytest.mark.parametrize("width,net,points,need_input", _halves_cases(),
                         ids=[f"w{w}-{n}-{p}-{'input' if i else 'noinput'}" for w, n, p, i in _halves_cases()])
def test_point_halves(dev, width, net, points, need_input):
    if need_input:
        LG._check(LG.run_case(dev, "f32", True, width, net, POINTS[points]))
    else:
        failures, _ = run_without_input_grad(dev, width, net, POINTS[points])
        assert not failures, "\n" + "\n".join(failures)


# ---------------------------------------------------------------------------------------------- 2. integers
INT_NETS = {"L3": (3, ()), "L4skip": (4, (2,))}
INT_CASES = [(w, n, layer) for w in (64, 256) for n, (L, _) in INT_NETS.items() for layer in range(L - 1)]
M_INF = 49  # a full wave tile and one that ends one row into its second point half


def _integer_net(width, layers, skips, base=_integer_field):
    """base (_integer_field: trunk x parts -2 .. 2 on eight rows a column, the raw-coordinate columns of the encoded parts, the density
    row) plus what the backward sweep crosses in front of the trunk and behind it: sparse -2 .. 2 on the sin / cos columns of the
    encoded parts (one row in sixteen), a bottleneck of two +-1 a row, one +-1 bottleneck unit per mlp_mid unit (so W_c = W_mid,x W_b
    is exact, two +-1 a row), integer biases there (b_c exact), and an RGB head of -1 / 0 / 1."""
    f = base(width, layers, skips)
    i, j = torch.arange(width)[:, None], torch.arange(width)[None, :]
    with torch.no_grad():
        for l in range(layers):
            if l == 0 or l in skips:
                c = torch.arange(96)[None, :]
                f.mlp_base.layers[l].weight[:, :96] = ((((3 * i + 5 * c + l) % 5) - 2) * (((i + 7 * c + l) % 16) == 0)).float()
        wb = f.field_output_bottleneck.net
        wb.weight.copy_(((((i + j) % 2) * 2 - 1) * (((j - 3 * i) % width) < 2)).float())
        wb.bias.copy_(torch.round(wb.bias * 8))
        mid = f.mlp_mid.layers[0]
        hj = torch.arange(128)[:, None]
        wm = mid.weight.clone()
        wm[:, 34:] = ((((hj % 2) * 2 - 1)) * (j == (5 * hj) % width)).float()
        mid.weight.copy_(wm)
        mid.bias.copy_(torch.round(mid.bias * 8))
        f.field_output_mid.net.weight.copy_((((torch.arange(3)[:, None] + torch.arange(128)[None, :]) % 3) - 1).float())
    return f


def _inf_forward(dev, f, inp, d_inf, sq, fold):
    n_dev = torch.tensor([M_INF], dtype=torch.int32, device=dev)
    with LG._launching():
        _, _, inf_saved = f.evaluate_reflect_train(inp["o"].to(dev), d_inf.to(dev), inp["pa"].to(dev), inp["eb"].to(dev), n_dev,
                                                   sq.to(dev), fold=fold)
        inf_saved["heads"][:, 4:7] = 0.5  # the mid colour behind its sigmoid: mid (1 - mid) = 1/4 exactly
    return inf_saved


def _inf_backward(dev, f, d_inf, sq, inf_saved, g_bg, need_input, fold):
    """rsn_field_backward_inf on poisoned gradient buffers -> gout on the host"""
    lib = pkg.load_library()
    gout, gst = (train_graph._alloc_gout_folded if fold else train_graph._alloc_gout)(f, M_INF, dev, need_input)
    _poisoned(gout)
    fs, desc, pk = ops.saved_struct(inf_saved), f.field_desc(fold), f.packed_weights(fold)
    d_dev, sq_dev, g_dev = d_inf.to(dev), sq.to(dev), g_bg.to(dev)
    with LG._launching():
        check(lib.rsn_field_backward_inf(C.byref(desc), ptr(pk), M_INF, None, ptr(d_dev), ptr(sq_dev), C.byref(fs), ptr(g_dev),
                                         C.byref(gst), 1 if need_input else 0, ops._stream()))
    return _host(gout)


@pytest.mark.parametrize("group", range(8))
@pytest.mark.parametrize("width,net,layer", INT_CASES, ids=[f"w{w}-{n}-mask{l}" for w, n, l in INT_CASES])
def test_integer_sums_row_halves_and_nibbles(dev, width, net, layer, group):
    layers, skips = INT_NETS[net]
    skip = skips[0] if skips else -1
    f = _integer_net(width, layers, skips)
    inside = ((torch.arange(width) % 32) // 4) == group
    with torch.no_grad():  # pre-activations of these integer layers stay far below 1e3: a unit outside the group is dead at every point
        f.mlp_base.layers[layer].bias[~inside] = -1e3
    f.to(dev).train()
    f.set_mma_mode("f32")
    inp = S._rays(M_INF, 2, seed=width + layers)
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    sq, d_inf = inf["sq"][:M_INF].contiguous(), inf["d"][:M_INF].contiguous()
    g = torch.Generator().manual_seed(width + 8 * layer + group)
    g_bg = 4.0 * torch.randint(-1, 2, (M_INF, 3), generator=g).float()
    folded, plain = _inf_forward(dev, f, inp, d_inf, sq, True), _inf_forward(dev, f, inp, d_inf, sq, False)
    act = folded["act"].cpu()
    assert torch.equal(act, plain["act"].cpu()) and torch.equal(folded["hid"].cpu() > 0, plain["hid"].cpu() > 0)
    live = act[layer][:, :width] > 0
    assert not bool(live[:, ~inside].any())
    frac = float(live[:, inside].float().mean())
    assert 0.05 < frac < 0.95, f"group {group} mask {frac:.2f} live: not a mixed mask"
    on = _inf_backward(dev, f, d_inf, sq, folded, g_bg, True, True)
    off = _inf_backward(dev, f, d_inf, sq, folded, g_bg, False, True)
    ref = _inf_backward(dev, f, d_inf, sq, plain, g_bg, True, False)
    dy = on["dy"].reshape(layers, M_INF, -1)
    assert bool(torch.isfinite(dy).all()) and bool((dy == dy.round()).all()), "the layer gradients are not integers"
    assert float(dy[layers - 1].abs().max()) > 0, "no gradient reaches the trunk: the case tells nothing"
    P = _host(f.state_dict())
    for l in range(layers - 1, 0, -1):
        w = P[f"mlp_base.layers.{l}.weight"].double()
        w = w[:, 99:] if l == skip else w
        x = dy[l][:, :width].double()
        assert float((x.abs() @ w.abs()).max()) * 1.01 ** 2 < 2.0 ** 24, "a partial sum may leave the exact range: not an exact case"
        want = (x @ w) * (act[l - 1][:, :width] > 0)
        assert torch.equal(dy[l - 1][:, :width].double(), want), f"dy[{l - 1}] differs from the host's integer sums"
        assert bool((dy[l - 1][:, width:] == 0).all())
    assert float(dy[layer].abs().max()) > 0, f"dy[{layer}] is all zero: the mask of the confined layer let nothing through"
    for other, name in ((off, "without the input gradient"), (ref, "of the unfolded instantiation")):
        assert torch.equal(other["dy"].reshape(dy.shape), dy), f"dy {name} differs"
    # d_input: the encoded-input sums are exact integers too (checked here against the host), the float32 chain behind them is
    # the code the unfolded instantiation runs
    g_enc_s = (dy[0][:, :width].double().abs() @ P["mlp_base.layers.0.weight"].double().abs()).max()
    if skip > 0:
        g_enc_s = g_enc_s + (dy[skip][:, :width].double().abs() @ P[f"mlp_base.layers.{skip}.weight"].double()[:, :99].abs()).max()
    assert float(g_enc_s) * 1.01 ** 2 < 2.0 ** 24
    assert bool(torch.isfinite(on["d_input"]).all()) and float(on["d_input"].abs().max()) > 0
    assert torch.equal(on["d_input"], ref["d_input"]), "d_input differs from the unfolded instantiation's on exact sums"


# ---------------------------------------------------------------------------------------------- 3. no stray stores
# (rays in the buffers, live rays), one sample a ray: the last live wave holds 1, 16, 17, 31 rows; 129: one row in a second tile
COUNTS = [(70, 33), (70, 48), (70, 49), (70, 63), (300, 129)]


@pytest.mark.parametrize("need_input", [True, False], ids=["input", "noinput"])
@pytest.mark.parametrize("cap,live", COUNTS, ids=[f"{c}-{l}" for c, l in COUNTS])
@pytest.mark.parametrize("width", WIDTHS)
def test_no_stray_stores(dev, width, cap, live, need_input):
    if need_input:
        LG._check(LG.run_case(dev, "f32", True, width, "L8", (cap, 1), n_live_rays=live))
    else:
        failures, _ = run_without_input_grad(dev, width, "L8", (cap, 1), n_live_rays=live)
        assert not failures, "\n" + "\n".join(failures)


# ---------------------------------------------------------------------------------------------- 4. multi-job launch
@pytest.mark.parametrize("width", [256, 64])
def test_jobs_launch_equals_separate_launches(dev, width):
    layers, skips = LG.NETS["L8"]
    M = 45
    f = S._field(width, layers=layers, skips=skips, seed=31)
    f.to(dev).train()
    f.set_mma_mode("f32")
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    sq, d_inf = inf["sq"][:M].contiguous().to(dev), inf["d"][:M].contiguous().to(dev)
    n_dev = torch.tensor([M], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(width)
    levels, inf_saved, rays = [], None, None
    with LG._launching():
        for Sn in (3, 2):
            inp = S._rays(M, Sn, seed=width + Sn)
            if rays is None:
                rays = (inp["o"].to(dev), d_inf, inp["pa"].to(dev))
            eb = inp["eb"].to(dev)
            lv, _, inf_saved = f.evaluate_reflect_train(*rays, eb, n_dev, sq, fold=True)
            levels.append((eb, lv, torch.randn(M, Sn, 3, generator=g).to(dev), Sn))
        g_bg = torch.randn(M, 3, generator=g).to(dev)
        gouts, gout_inf = train_graph._reflect_field_backward(f, rays, sq, levels, inf_saved, g_bg, n_dev, M, fold=True)
        single = [train_graph._field_backward(f, rays, eb, lv, {"color": gc.reshape(-1, 3)}, True, n_dev=n_dev, fold=True)
                  for eb, lv, gc, _ in levels]
    for k, (a, b) in enumerate(zip(gouts, single)):
        for key in ("dy", "da_mid", "dz_rgb", "dz_heads", "d_input"):
            assert bool(torch.isfinite(a[key]).all()), f"level {k} {key}"
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), f"level {k} {key}: the jobs launch differs from the single call"
    lib = pkg.load_library()
    go, gst = train_graph._alloc_gout_folded(f, M, dev, True)
    fs, desc, pk = ops.saved_struct(inf_saved), f.field_desc(True), f.packed_weights(True)
    with LG._launching():
        check(lib.rsn_field_backward_inf(C.byref(desc), ptr(pk), M, ptr(n_dev), ptr(d_inf), ptr(sq), C.byref(fs), ptr(g_bg), C.byref(gst),
                                         1, ops._stream()))
    for key in ("dy", "da_mid", "d_input"):
        assert torch.equal(gout_inf[key].view(torch.int32), go[key].view(torch.int32)), f"get_inf_color {key}: the jobs launch differs from the single call"


# ---------------------------------------------------------------------------------------------- 5. repeatability
@pytest.mark.parametrize("width,net,points", [(256, "L8", "300"), (64, "L3", "49")])
def test_two_runs_are_bit_equal(dev, width, net, points):
    (fa, a), (fb, b) = (run_without_input_grad(dev, width, net, POINTS[points]) for _ in range(2))
    assert not fa and not fb
    for key in a:
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), f"{key} differs between two runs"
