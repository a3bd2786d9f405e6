"""The analytic normals of the exact-fp32 training forward once every GEMM of the sweep runs on the bf16 MFMAs: behind the peeled
seed GEMM, W_l^T for l = L-2 .. 1 and the two encoded-input GEMMs take all nine products of three bf16 pieces a side (rsn_gemm_loops.h:
gemm_bf16<.., 3, true> over the packed hT_* segments in the folded instantiation, gemm_f32_x9 with the pieces formed in registers in
the unfolded one).

The reference and the rule are those of tests/test_normals_seed_gpu.py: the sweep restated in fp64 on the kernel's own masks, means
and float32 phases, judged by field_maths_reference.compare with its existing bounds.  The shapes are the ones at which the new loop
takes another path:

  width 32 and 64 run the 64-wide kernel (32: zero-padded units), whose W x W loop has one block per fragment half and whose
  encoded-input loop has two; 128 has two / two; 256 four / two;
  L = 2 runs the peeled GEMM alone (plus the last encoded-input GEMM), L = 3 one nine-product W x W GEMM without a skip layer,
  L = 6 and 8 have the skip layer live: the skip's encoded-input GEMM sits inside the loop;
  1 point (one lane of one wave), 33 points (a second wave with one valid row), 128 * CUs + 33 points (the persistent loop of
  the workgroups turns over; the last tile is ragged)."""
import pytest
import torch

import reflect_sampling_nerf_amd as pkg  # noqa: F401
from tests import field_maths_reference as R  # noqa: F401
from tests import test_normals_seed_gpu as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


NETS = {"L2": (2, ()), "L3": (3, ()), "L6": (6, (4,)), "L8": (8, (4,))}
# (width, net, points): every width x every depth at 33 points; the one-point and multi-pass shapes at the narrowest and the widest
# kernel (multi-pass at 256 on the three-layer net: the saved rows of 33 k points come back to the host for the reference)
CASES = [(w, n, "33") for w in (32, 64, 256) for n in NETS] + [
    (128, "L8", "33"), (64, "L8", "1"), (256, "L8", "1"), (64, "L8", "multipass"), (256, "L3", "multipass")]


def _points(name):
    """(rays, samples per ray) of a point count"""
    if name == "multipass":
        return 128 * torch.cuda.get_device_properties(0).multi_processor_count + 33, 1
    return {"1": (1, 1), "33": (11, 3)}[name]


def _skip(skips):
    return skips[0] if skips else -1


@pytest.mark.parametrize("width,net,points", CASES, ids=[f"w{w}-{n}-{p}" for w, n, p in CASES])
def test_normals_against_the_fp64_sweep(dev, width, net, points):
    """Both exact-fp32 instantiations within the rule of the fp64 sweep, and bit-equal to one another: the packed pieces and the
    pieces formed in registers are the same bf16 values and meet each accumulator in the same order."""
    layers, skips = NETS[net]
    Rn, Sn = _points(points)
    f, inp = S._field(width, layers=layers, skips=skips, seed=11), S._rays(Rn, Sn, seed=width + layers + Rn)
    (n0, act0, m0), (n1, act1, m1) = (S._run(dev, f, inp, fold) for fold in (False, True))
    assert n0.shape == (Rn * Sn, 3) and bool(torch.isfinite(n0).all())
    assert torch.equal(act0, act1) and torch.equal(m0, m1)
    assert torch.equal(n0, n1), "folded and unfolded normals differ"
    ref, ora = S._references(f, layers, _skip(skips), inp, act0, m0)
    S._judge(f"w{width} {net} {points}", n0, ref, ora)


def _integer_field(width, layers, skips):
    """Small integer weights in every layer the sweep crosses.  Trunk layers l >= 1: values -2 .. 2, distinct along both axes, kept
    on eight rows of each column (a K permutation or a swapped piece changes the sums); the encoded-input parts (layer 0, the skip
    layer) read the three raw coordinates alone, through -2 .. 2, so the gradient leaves the sweep on the raw-coordinate columns and
    the sin / cos columns carry exact zeros.  The biases keep random values: the masks are mixed.
    Bound on every partial sum, products of pieces included (the pieces of an integer are integers, and the sum of their magnitudes
    is below 1.01 times the value's): the density row is below 4, so the peeled GEMM gives at most 4 * 2 * 8 = 64, every further
    W x W GEMM multiplies by at most 2 * 8 = 16 (two of them at L = 4: 16,384), and an encoded-input GEMM by at most 2 * width = 512:
    8.4e6 * 1.01^2 < 2^24.  Every sum is an integer that fp32 holds exactly, in any order."""
    f = S._field(width, layers=layers, skips=skips, seed=5)
    keep = max(1, width // 8)
    i = torch.arange(width, dtype=torch.float32)[:, None]
    with torch.no_grad():
        for l in range(layers):
            lin = f.mlp_base.layers[l]
            in_f = lin.weight.shape[1]
            w = torch.zeros(width, in_f)
            if l == 0 or l in skips:
                w[:, 96:99] = ((3 * i + 7 * torch.arange(3.0)[None, :] + l) % 5) - 2
            if l >= 1:
                j = torch.arange(width, dtype=torch.float32)[None, :]
                w[:, in_f - width:] = ((((7 + l) * i + 13 * j) % 5) - 2) * (((i + 3 * j + l) % keep) == 0)
            lin.weight.copy_(w)
            lin.bias.mul_(20.0 if l == 0 else 200.0)
        f.field_output_density.net.weight.copy_((((5 * i[:, 0]) % 9) - 4).reshape(1, width))
    return f


@pytest.mark.parametrize("width", [256, 64, 32])
@pytest.mark.parametrize("net", ["L3", "L4skip"])
def test_integer_weights_pin_the_nine_products(dev, width, net):
    """With these weights the encoded-input gradient is exact whatever the order of the accumulation, so the direction equals the
    fp64 one up to the normalisation (three squares, a square root and a division in fp32): 1e-6, the seed test's bound, which no
    tolerance of the GEMMs enters.  A dropped, doubled or misplaced piece product gives another integer vector."""
    layers, skips = {"L3": (3, ()), "L4skip": (4, (2,))}[net]
    f, inp = _integer_field(width, layers, skips), S._rays(37, 3, seed=width + layers)
    for fold in (False, True):
        got, act, means = S._run(dev, f, inp, fold)
        W = f.field_output_density.net.weight.shape[1]
        for l in range(layers):
            live = float((act[l][:, :W] > 0).float().mean())
            assert 0.05 < live < 0.95, f"layer {l} mask {live:.2f} live: not a mixed mask"
        ref, ora = S._references(f, layers, _skip(skips), inp, act, means)
        err = float((got.double() - ref).abs().max())
        print(f"[w{width} {net} fold={fold}] integer weights: worst |normals - fp64| {err:.3e} "
              f"(the float32 sweep: {float((ora.double() - ref).abs().max()):.3e})")
        assert float((ref.norm(dim=-1) > 0.5).float().mean()) > 0.9  # (a zero integer gradient sits on the 1e-12 clamp: 0 on both sides)
        assert err <= 1e-6


@pytest.mark.parametrize("width", [256, 64])
def test_all_live_and_all_dead_masks(dev, width):
    """The mask between the peeled GEMM and the first nine-product GEMM (layer L-2).  Bias +large: every bit set, the nine-product
    GEMM sums whole rows.  -large: none set, its operand is exactly zero, and the normals are exactly 0 through the 1e-12 clamp."""
    inp = S._rays(37, 3, seed=width + 2)
    for sign in (1.0, -1.0):
        f = S._field(width, seed=7)
        with torch.no_grad():
            f.mlp_base.layers[6].bias.fill_(sign * 1e3)
        for fold in (False, True):
            got, act, means = S._run(dev, f, inp, fold)
            W = f.param_width
            assert bool(((act[6][:, :W] > 0) == (sign > 0)).all())
            if sign < 0:
                assert bool((got == 0).all())
            else:
                ref, ora = S._references(f, 8, 4, inp, act, means)
                S._judge(f"w{width} layer 6 all live fold={fold}", got, ref, ora)


def worst_error(dev, fold=True):
    """The 8 x 256 field on 128 rays x 32 samples: (normals, fp64 reference, float32 restatement) of the library in use"""
    f, inp = S._field(256, seed=3), S._rays(128, 32, seed=256 + 3)
    got, act, means = S._run(dev, f, inp, fold)
    ref, ora = S._references(f, 8, 4, inp, act, means)
    return got, ref, ora


def test_error_at_the_headline_width(dev):
    """The figure profiles/normals_x9.json records beside the parent build's (tools/normals_x9_error.py): printed here, and held
    to the same rule as every other shape."""
    got, ref, ora = worst_error(dev)
    print(f"[8 x 256, 4096 points] worst |normals - fp64| {float((got.double() - ref).abs().max()):.3e} "
          f"(the float32 sweep: {float((ora.double() - ref).abs().max()):.3e})")
    S._judge("w256 L8 4096 points", got, ref, ora)
