"""The nine-product GEMMs of the analytic-normal sweep on the 16x16x32 bf16 MFMA shape (rsn_gemm_loops.h: gemm_bf16_s16 over the packed
hT_* segments in the folded instantiation, gemm_f32_x9_s16 with the pieces formed in registers in the unfolded one).

tests/test_normals_x9_gpu.py, test_normals_seed_gpu.py and test_fold_bottleneck_gpu.py judge the loop as they judged the 32x32x16
one.  Here is only what the new lane mapping can get wrong and their shapes do not reach.  A wave's 32-point tile is now two point
halves of 16, a 32-row block two row halves of 16, and a lane writes, per result, one float4 of ANOTHER lane's slot of the LDS slab
under a nibble of that other lane's mask words:

  point halves: 16, 17, 31, 32 and 49 points -- the second point half of the tile empty, with one row, lacking one row, full, and
  a second wave that starts in a half -- at width 64 (two blocks: one fragment buffer per block) and 256 (eight: two blocks per
  buffer), on the three-layer net (one nine-product W x W GEMM) and the eight-layer one (six, the skip layer's GEMM among them);

  row halves and nibbles: integer weights (every sum exact in fp32 in any order), the live units of the layer whose mask the new
  epilogue applies confined by its biases to ONE 4-row group of every 32-row block, for each of the eight groups in turn: group
  2 q + h of the 32x32 layout is row half q >> 1, lane group 2 (q & 1) + h of the 16x16 one.  A wrong nibble, row half or lane
  pick masks the live rows away or lets dead ones through: another integer vector.

The reference and the rule are those of tests/test_normals_seed_gpu.py, imported, and folded and unfolded are bit-equal in every
case."""
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from tests import test_normals_seed_gpu as S
from tests.test_normals_x9_gpu import NETS, _integer_field, _skip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


def _both(dev, f, inp):
    """(normals, saved activations, means) of the unfolded run, after checking that the folded one has the same bits"""
    (n0, act0, m0), (n1, act1, m1) = (S._run(dev, f, inp, fold) for fold in (False, True))
    assert bool(torch.isfinite(n0).all())
    assert torch.equal(act0, act1) and torch.equal(m0, m1)
    assert torch.equal(n0, n1), "folded and unfolded normals differ"
    return n0, act0, m0


@pytest.mark.parametrize("points", [16, 17, 31, 32, 49])
@pytest.mark.parametrize("net", ["L3", "L8"])
@pytest.mark.parametrize("width", [64, 256])
def test_point_halves(dev, width, net, points):
    layers, skips = NETS[net]
    f, inp = S._field(width, layers=layers, skips=skips, seed=13), S._rays(points, 1, seed=width + layers + points)
    got, act, means = _both(dev, f, inp)
    assert got.shape == (points, 3)
    ref, ora = S._references(f, layers, _skip(skips), inp, act, means)
    S._judge(f"w{width} {net} {points} points", got, ref, ora)


# (net, the layer whose mask the 16-shape epilogue applies): on L3 the only nine-product W x W GEMM is W_1^T, masked by layer 0;
# on L4skip W_2^T, whose result the mask of layer 1 meets between two nine-product GEMMs (W_1^T reads it), is the first
MASKED = {"L3": 0, "L4skip": 1}


@pytest.mark.parametrize("group", range(8))
@pytest.mark.parametrize("net", list(MASKED))
@pytest.mark.parametrize("width", [64, 256])
def test_row_halves_and_nibbles(dev, width, net, group):
    """The direction equals the fp64 one up to the normalisation: 1e-6, the bound of the integer tests of the seed and the
    nine-product files (three squares, a square root and a division in fp32; no tolerance of the GEMMs enters)."""
    layers, skips = {"L3": (3, ()), "L4skip": (4, (2,))}[net]
    f, inp = _integer_field(width, layers, skips), S._rays(37, 3, seed=width + layers)
    layer = MASKED[net]
    units = torch.arange(width)
    inside = ((units % 32) // 4) == group
    with torch.no_grad():  # pre-activations of these integer layers stay far below 1e3: a unit outside the group is dead at every point
        f.mlp_base.layers[layer].bias[~inside] = -1e3
    got, act, means = _both(dev, f, inp)
    W = f.field_output_density.net.weight.shape[1]
    live = act[layer][:, :W] > 0
    assert not bool(live[:, ~inside].any())
    frac = float(live[:, inside].float().mean())
    assert 0.05 < frac < 0.95, f"group {group} mask {frac:.2f} live: not a mixed mask"
    ref, ora = S._references(f, layers, _skip(skips), inp, act, means)
    err = float((got.double() - ref).abs().max())
    moving = float((ref.norm(dim=-1) > 0.5).float().mean())
    print(f"[w{width} {net} group {group}] worst |normals - fp64| {err:.3e} (the float32 sweep: "
          f"{float((ora.double() - ref).abs().max()):.3e}), {moving:.2f} of the points with a non-zero gradient")
    assert moving > 0.25  # (a zero integer gradient sits on the 1e-12 clamp, 0 on both sides: it tells nothing about the mask)
    assert err <= 1e-6
