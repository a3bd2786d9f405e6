"""The analytic normals of the exact-fp32 training forward (evaluate_frustums_train on one primary level), whose sweep starts on the
bf16 MFMAs from the ReLU bits of the last trunk layer against the seed segment hT_seed (gemm_bf16_bits, rsn_gemm_loops.h).

The reference is an fp64 restatement of the sweep on the kernel's own numbers -- its ReLU masks (saved activations > 0), its
contracted means (the raw-coordinate slots of the saved encoded inputs) and the float32 IPE phases of tests/field_maths_reference.py
-- so a point near a ReLU kink or an undamped top frequency does not turn a rounding difference into a different function.  The
rule is field_maths_reference.compare, the one tests/test_field_maths_gpu.py judges rows by: the kernel's worst error may be FACTOR
times the worst error of the SAME restatement evaluated in float32, plus one ulp."""
import math

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from tests import field_maths_reference as R

pytestmark = pytest.mark.gpu

# 37 x 3: 111 points, the last wave of the tile has 15 valid rows.  997 x 33 = 257 x 128 + 5 points: more 128-point tiles than
# workgroups, so the persistent loop turns over, and the last tile has one wave with 5 rows
SHAPES = {"ragged": (37, 3), "multipass": (997, 33)}
WIDTHS = [256, 128, 64, 200]  # 200: zero-padded units inside 256


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


def _field(width, layers=8, skips=(4,), seed=0):
    torch.manual_seed(1000 + seed + width)
    f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=layers, base_mlp_layer_width=width, skip_connections=skips)
    with torch.no_grad():
        f.field_output_density.net.bias += 1.0
    return f


def _rays(Rn, S, seed, area_exp=(-4.0, -2.0)):
    g = torch.Generator().manual_seed(seed)
    o, d, _ = cpu_ref.synthetic_rays(Rn, seed=seed)
    pa = 10.0 ** (area_exp[0] + (area_exp[1] - area_exp[0]) * torch.rand(Rn, 1, generator=g))
    _, eb = cpu_ref.spaced_bins("uniform", 1.0, torch.full((Rn, 1), 2.0), torch.full((Rn, 1), 6.0), S, torch.rand(Rn, S + 1, generator=g))
    return {"o": o, "d": d, "pa": pa.reshape(Rn), "eb": eb.contiguous()}


def _run(dev, f, inp, fold):
    f.to(dev).train()
    f.set_mma_mode("f32")
    lv = f.evaluate_frustums_train(inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev), inp["eb"].to(dev), want_normals=True, fold=fold)
    torch.cuda.synchronize()
    lay = f.train_layout()
    means = lv["saved"]["enc"][:, [lay["enc_map"].index(96 + c) for c in range(3)]]
    return lv["normals"].reshape(-1, 3).cpu(), lv["saved"]["act"].cpu(), means.cpu()


def sweep(P, layers, skip, act, mean32, var, dtype):
    """-normalize(d raw_density / d mean) in `dtype`: the density row masked by the last layer's ReLU, back through the trunk
    (the skip layer's encoded-input part adds to the encoded-input gradient), then through sin(phase) exp(-var f^2 / 2) with the
    float32 phases taken as exact (d phase / d mean = 2 pi f) and the variance a constant, as the reference detaches it."""
    W = P["field_output_density.net.weight"].shape[1]
    mask = (act[:, :, :W] > 0).to(dtype)
    w = lambda l: P[f"mlp_base.layers.{l}.weight"].to(dtype)  # noqa: E731
    g = P["field_output_density.net.weight"].to(dtype).reshape(1, W) * mask[layers - 1]
    g_enc = torch.zeros(act.shape[1], 99, dtype=dtype)
    for l in range(layers - 1, 0, -1):
        wl = w(l)
        if l == skip:
            g_enc = g_enc + g @ wl[:, :99]
            wl = wl[:, 99:]
        g = (g @ wl) * mask[l - 1]
    g_enc = g_enc + g @ w(0)
    freqs32 = R.frequencies()
    ps, pc = R.phases(mean32, freqs32)
    f = freqs32.to(dtype)
    damp = torch.exp(-0.5 * (var.to(dtype)[..., None] * f ** 2).reshape(var.shape[0], -1))
    per = (g_enc[:, :48] * (damp * torch.cos(ps.to(dtype))) + g_enc[:, 48:96] * (damp * torch.cos(pc.to(dtype)))) * f.repeat(3)
    grad = 2 * math.pi * per.reshape(-1, 3, 16).sum(-1) + g_enc[:, 96:99]
    return -(grad / grad.norm(dim=-1, keepdim=True).clamp_min(1e-12))


def _references(f, layers, skip, inp, act, means):
    P = {k: v.detach().cpu() for k, v in f.state_dict().items()}
    out = []
    for dtype in (torch.float64, torch.float32):
        var = R.gaussian({**inp, "pa": inp["pa"].reshape(-1, 1)}, dtype)[1]
        out.append(sweep(P, layers, skip, act, means, var, dtype))
    return out


def _judge(label, got, ref, ora):
    v = R.compare(label, "normals", got, ref, ora, torch.zeros(got.shape[0], dtype=torch.long), ["all"])
    print(v.report())
    assert v.ok, v.report()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("width", WIDTHS)
def test_normals_against_the_fp64_sweep(dev, width, shape):
    """Ragged and multi-pass shapes at every width, through both exact-fp32 instantiations: each within the rule of the fp64 sweep,
    and bit-equal to one another (they run the same sweep on the same bits)."""
    Rn, S = SHAPES[shape]
    f, inp = _field(width), _rays(Rn, S, seed=width + Rn)
    res = {fold: _run(dev, f, inp, fold) for fold in (False, True)}
    (n0, act0, m0), (n1, act1, m1) = res[False], res[True]
    assert bool(torch.isfinite(n0).all()) and torch.equal(act0, act1) and torch.equal(m0, m1)
    assert torch.equal(n0, n1), "folded and unfolded normals differ"
    ref, ora = _references(f, 8, 4, inp, act0, m0)
    _judge(f"w{width} {shape}", n0, ref, ora)


def _integer_field(width):
    """Two trunk layers, no skip.  The last trunk layer and the density row hold small integers, distinct along both axes (a K
    permutation or a swapped piece changes the sums); layer 0 reads the three raw coordinates alone, through small integers too,
    so the gradient leaves the sweep on the raw-coordinate columns and the sin / cos columns carry exact zeros.  The biases keep
    random values: the masks are mixed.  Every product and partial sum of both GEMMs is an integer below 2^24, exact in fp32 in any
    order, and the un-normalised gradient is an integer vector."""
    f = _field(width, layers=2, skips=(), seed=5)
    n = torch.arange(width, dtype=torch.float32)
    with torch.no_grad():
        w0 = torch.zeros(width, 99)
        w0[:, 96:] = ((3 * n[:, None] + 7 * torch.arange(3.0)[None, :]) % 5) - 2
        f.mlp_base.layers[0].weight.copy_(w0)
        f.mlp_base.layers[1].weight.copy_(((7 * n[:, None] + 13 * n[None, :]) % 11) - 5)
        f.field_output_density.net.weight.copy_((((5 * n) % 9) - 4).reshape(1, width))
        f.mlp_base.layers[0].bias.mul_(20.0)
        f.mlp_base.layers[1].bias.mul_(200.0)
    return f


@pytest.mark.parametrize("width", [256, 128, 64])
def test_integer_weights_pin_the_layout(dev, width):
    """With these weights the sweep is exact up to the normalisation (three squares, a square root and a division in fp32), so the
    direction equals the fp64 one to 1e-6 -- a bound no tolerance of the GEMMs enters.  A wrong K order or piece order gives another
    integer vector.  (With sin / cos columns in play the float32 restatement of the closing chain is itself 1.5e-6 from fp64 at
    width 256, through the fp32 variance in the damping: that part is judged by the rule above, not here.)"""
    f, inp = _integer_field(width), _rays(37, 3, seed=width + 1)
    for fold in (False, True):
        got, act, means = _run(dev, f, inp, fold)
        live = (act[1] > 0).float().mean()
        assert 0.1 < float(live) < 0.9, f"last-layer mask {float(live):.2f} live: not a mixed mask"
        ref, ora = _references(f, 2, -1, inp, act, means)
        err = float((got.double() - ref).abs().max())
        print(f"[w{width} fold={fold}] integer weights: worst |normals - fp64| {err:.3e} (the float32 sweep: {float((ora.double() - ref).abs().max()):.3e})")
        assert bool((ref.norm(dim=-1) > 0.5).all())  # no point sits on the 1e-12 clamp
        assert err <= 1e-6


@pytest.mark.parametrize("width", [256, 64])
def test_all_live_and_all_dead_masks(dev, width):
    """Last-layer bias +large: every bit set (the seed GEMM sums all of V).  -large: none set, the gradient is exactly zero and the
    normals are exactly 0 through the 1e-12 clamp."""
    inp = _rays(37, 3, seed=width + 2)
    for sign in (1.0, -1.0):
        f = _field(width, seed=7)
        with torch.no_grad():
            f.mlp_base.layers[7].bias.fill_(sign * 1e3)
        for fold in (False, True):
            got, act, means = _run(dev, f, inp, fold)
            W = f.param_width
            assert bool(((act[7][:, :W] > 0) == (sign > 0)).all()) and bool((act[7][:, W:] == 0).all())
            if sign < 0:
                assert bool((got == 0).all())
            else:
                ref, ora = _references(f, 8, 4, inp, act, means)
                _judge(f"w{width} all live fold={fold}", got, ref, ora)
