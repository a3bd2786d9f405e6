"""Host-side companion of tests/test_depth_skip_gpu.py: every case of that file is shown to be meaningful before a GPU sees it (no
layer of a random net dead or saturated, every integer case inside the exact range with mixed masks and a gradient at more than
0.9 of its points), and the host-only layout calls accept every trunk depth 1 .. 16 with every skip position, and refuse the rest
with the messages of rsn_compute_layout."""
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi
from reflect_sampling_nerf_amd._build import build_library
from tests import depth_skip_cases as D
from tests import field_maths_reference as R
from tests import test_backward_x9_gpu as TB
from tests.helpers import default_dtype

f64 = torch.float64


# ---------------------------------------------------------------------------------------------- the cases of the GPU file
def test_the_nets_are_the_thirteen_classes():
    assert len(D.NETS) == 13 and D.NETS["L1"] == (1, ()) and D.NETS["L16s14"] == (16, (14,))
    for net, (layers, skips) in D.NETS.items():
        assert 1 <= layers <= _abi.RSN_MAX_TRUNK_LAYERS and len(skips) <= 1
        assert not skips or 1 <= skips[0] <= layers - 2, net
    cases = D.random_cases()
    for family in ("f32", "bf16x6", "bf16"):  # every net at width 256 in every family; the nets over the ring's limit among them
        assert {n for fa, _, w, n, p in cases if fa == family and w == 256 and p == "33"} == set(D.NETS)
    assert {n for n, (layers, _) in D.NETS.items() if layers > D.RING_MAX_LAYERS} == {"L11s4", "L16s1", "L16s14"}


RANDOM_SHAPES = sorted({(w, n, p) for _, _, w, n, p in D.random_cases()})


@pytest.mark.parametrize("width,net,points", RANDOM_SHAPES, ids=[f"w{w}-{n}-{p}" for w, n, p in RANDOM_SHAPES])
def test_no_layer_of_a_random_case_is_dead_or_saturated(width, net, points):
    layers, skips = D.NETS[net]
    shares = D.live_shares(D.random_field(width, layers, skips), layers, skips, D.case_rays(width, layers, points))
    print(f"[w{width} {net} {points}] live shares: " + " ".join(f"{s:.2f}" for s in shares))
    D.assert_live(f"w{width} {net} {points}", shares)


INT_ALL = [(w, n) for w in D.INT_WIDTHS for n in D.ALL]


@pytest.mark.parametrize("width,net", INT_ALL, ids=[f"w{w}-{n}" for w, n in INT_ALL])
def test_integer_normal_sweep_case_is_exact_and_mixed(width, net):
    """sweep_sums asserts every partial sum times 1.01^2 below 2^24; the masks are mixed and > 0.9 of the points carry a gradient."""
    layers, skips = D.NETS[net]
    f, _, masks, grad = D.normal_sweep_case(width, net)
    D.assert_normal_sweep_case(f"w{width} {net}", masks, grad)
    if skips:  # the two encoded-input parts hold different integers: mistaking one for the other changes the vector
        w0, ws = f.mlp_base.layers[0].weight[:, 96:99], f.mlp_base.layers[skips[0]].weight[:, 96:99]
        assert not torch.equal(w0, ws)
    for l in range(1, layers):  # signed permutations but at the skip layer, above it, or at the top of a net without a skip
        w = f.mlp_base.layers[l].weight.detach()
        wx = w[:, w.shape[1] - width:]
        if l in D.dense_layers(layers, skips):
            assert int((wx != 0).sum(0).max()) <= 8 and float(wx.abs().max()) == 2.0
        else:
            assert bool(((wx != 0).sum(0) == 1).all()) and bool(((wx != 0).sum(1) == 1).all()) and float(wx.abs().max()) == 1.0
            assert float(wx.min()) == -1.0


@pytest.mark.parametrize("width,net", [c for c in INT_ALL if c[1] != "L1"], ids=[f"w{w}-{n}" for w, n in INT_ALL if n != "L1"])
def test_integer_forward_case_is_exact_and_mixed(width, net):
    layers, skips = D.NETS[net]
    z = D.forward_sums(f"w{width} {net}", D.forward_field(width, layers, skips, seed=width + layers), layers, skips)
    assert len(z) == layers and all(bool((t == t.round()).all()) for t in z)


@pytest.mark.parametrize("width,net", INT_ALL, ids=[f"w{w}-{n}" for w, n in INT_ALL])
def test_integer_backward_case_is_exact_and_mixed(width, net):
    """Worst case over every mask: |dz_rgb| <= 1 a column, so |da_mid| <= the RGB head's column sums, and every GEMM of the sweep
    multiplies the bound by its largest column sum of magnitudes: all below 2^24 / 1.01^2.  The masks of get_inf_color's job, from
    the fp64 forward on its inputs, are mixed in every layer."""
    layers, skips = D.NETS[net]
    skip = D.skip_of(skips)
    f = TB._integer_net(width, layers, skips, base=D.integer_field)
    P = {k: v.detach().double() for k, v in f.state_dict().items()}
    bound = float(P["field_output_mid.net.weight"].abs().sum(0).max())
    wc = P["mlp_mid.layers.0.weight"][:, 34:] @ P["field_output_bottleneck.net.weight"]
    assert bool((wc == wc.round()).all())
    bound *= float(wc.abs().sum(0).max())
    enc_bound = 0.0
    for l in range(layers - 1, 0, -1):
        w = P[f"mlp_base.layers.{l}.weight"]
        if l == skip:
            enc_bound += bound * float(w[:, :99].abs().sum(0).max())
            w = w[:, 99:]
        bound *= float(w.abs().sum(0).max())
        assert bound * D.PIECES < D.EXACT, f"layer {l}"
    enc_bound += bound * float(P["mlp_base.layers.0.weight"].abs().sum(0).max())
    assert enc_bound * D.PIECES < D.EXACT
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    mean, var = R.inf_gaussian({"d": inf["d"][:TB.M_INF], "sq": inf["sq"][:TB.M_INF]}, f64)
    with default_dtype(f64):
        enc = cpu_ref.ipe(cpu_ref.FieldSpec(), mean, var)
    shares = [float((z > 0).double().mean()) for z in D.trunk(P, layers, skip, enc)]
    for l, s in enumerate(shares):
        assert D.LIVE[0] < s < D.LIVE[1], f"layer {l} mask {s:.3f} live: not a mixed mask"


# ---------------------------------------------------------------------------------------------- the layout calls
@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


MODES = (_abi.RSN_MMA_F32, _abi.RSN_MMA_BF16X6, _abi.RSN_MMA_BF16X3, _abi.RSN_MMA_BF16, _abi.RSN_MMA_F32_FOLDED)


def _desc(layers, skip, width, mode):
    d = _abi.FieldDesc()
    d.num_layers, d.width, d.skip_layer, d.mid_width, d.density_bias, d.mma_mode, d.param_width = layers, width, skip, 128, 0.5, mode, 0
    return d


def _layout(lib, d):
    enc_cols, sh_cols, narrow = C.c_int32(), C.c_int32(), C.c_int32()
    enc_map, sh_map = (C.c_int32 * 128)(), (C.c_int32 * 64)()
    rc = lib.rsn_train_saved_layout(C.byref(d), C.byref(enc_cols), C.byref(sh_cols), C.byref(narrow), enc_map, sh_map)
    return rc, enc_cols.value, sh_cols.value, narrow.value, list(enc_map)[:enc_cols.value]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", [64, 128, 256])
def test_every_depth_and_skip_position_is_laid_out(lib, width, mode):
    """L = 1 .. 16, skip in {-1, 1 .. L-2}: both calls succeed; the bytes grow strictly with L at a fixed skip state; a live skip
    adds the same amount wherever it sits; the ring's saved-row layout is reported exactly up to ten layers (bf16 modes, width 256)."""
    plain, skipped = {}, {}
    for layers in range(1, _abi.RSN_MAX_TRUNK_LAYERS + 1):
        for skip in [-1] + list(range(1, layers - 1)):
            d = _desc(layers, skip, width, mode)
            nbytes = lib.rsn_packed_weights_bytes(C.byref(d))
            assert nbytes > 0 and nbytes % 4 == 0, (layers, skip, lib.rsn_last_error())
            rc, enc_cols, sh_cols, narrow, enc_map = _layout(lib, d)
            assert rc == 0, (layers, skip, lib.rsn_last_error())
            ring = mode in (_abi.RSN_MMA_BF16, _abi.RSN_MMA_BF16X6) and width == 256 and layers <= D.RING_MAX_LAYERS
            assert (enc_cols, sh_cols) == ((128, 64) if ring else (104, 40)), (layers, skip, enc_cols, sh_cols)
            assert narrow == int(ring and mode == _abi.RSN_MMA_BF16)
            assert sorted(c for c in enc_map if c >= 0) == list(range(99))
            if skip < 0:
                plain[layers] = nbytes
            else:
                skipped.setdefault(layers, set()).add(nbytes)
    for layers in range(2, _abi.RSN_MAX_TRUNK_LAYERS + 1):
        assert plain[layers] > plain[layers - 1]
    extra = {layers: v for layers, v in skipped.items()}
    assert set(extra) == set(range(3, _abi.RSN_MAX_TRUNK_LAYERS + 1))
    assert all(len(v) == 1 for v in extra.values()), "a live skip's bytes depend on where it sits"
    assert len({next(iter(v)) - plain[layers] for layers, v in extra.items()}) == 1, "a live skip's bytes depend on the depth"
    assert next(iter(extra[3])) > plain[3]
    for layers in range(4, _abi.RSN_MAX_TRUNK_LAYERS + 1):
        assert next(iter(extra[layers])) > next(iter(extra[layers - 1]))


@pytest.mark.parametrize("mode", MODES)
def test_what_the_layout_refuses(lib, mode):
    for layers in (1, 2, 3, 8, 16):
        for skip in (0, layers - 1, layers):
            if skip == -1:
                continue
            d = _desc(layers, skip, 256, mode)
            assert lib.rsn_packed_weights_bytes(C.byref(d)) == 0
            msg = lib.rsn_last_error().decode()
            assert f"skip_layer={skip} invalid for num_layers={layers}" in msg and "the skip index is the last layer" in msg.replace("\n", " "), msg
            assert _layout(lib, d)[0] != 0
    for layers in (0, 17):
        d = _desc(layers, -1, 256, mode)
        assert lib.rsn_packed_weights_bytes(C.byref(d)) == 0
        assert f"num_layers={layers} out of range [1,16]" in lib.rsn_last_error().decode()
        assert _layout(lib, d)[0] != 0


def test_a_skip_at_the_last_layer_reaches_the_caller_as_rsn_error(lib):
    """skip_connections=(4,) on five layers: nerfstudio's MLP accepts the constructor and raises a shape error in forward; the
    Field hands the library skip = L-1, and the library's refusal comes back as RsnError with its text."""
    f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=5, base_mlp_layer_width=64, skip_connections=(4,))
    d = f.field_desc()
    assert (d.num_layers, d.skip_layer) == (5, 4)
    with pytest.raises(_abi.RsnError, match=r"skip_layer=4 invalid for num_layers=5 \(the reference MLP raises a shape error"):
        f.train_layout()
    assert lib.rsn_packed_weights_bytes(C.byref(d)) == 0  # what packed_weights() turns into the same RsnError (check(-1))
    with pytest.raises(_abi.RsnError, match="skip_layer=4 invalid for num_layers=5"):
        _abi.check(-1)
