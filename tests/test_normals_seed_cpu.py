"""The seed segment of the analytic-normal sweep (hT_seed, rsn_pack.hip) without a GPU: the packed buffers keep their sizes -- the
segment takes the slot of hT_x[L-1] in the folded buffer, which the exact-fp32 modes leave unused -- and a numpy restatement of the three-piece bf16
split its exactness rests on: hi + mid + lo == x bit for bit, except below the documented underflow limit."""
import ctypes as C

import numpy as np
import pytest

import reflect_sampling_nerf_amd as pkg
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
def test_seed_segment_takes_no_room(lib, width, param_width):
    """The exact-fp32 buffer is as long as the buffer of a split-bf16 mode without the ring stream (RSN_MMA_BF16X3: every split copy
    written, hT_x[L-1] among them, 3 * (nb * 2) * nb * 256 floats -- the seed's size), for one trunk layer too, where there is no
    seed; the folded buffer is that plus the folded segments (tests/test_fold_bottleneck_cpu.py states them)."""
    for layers, skip in ((8, 4), (2, -1), (1, -1)):
        plain = lib.rsn_packed_weights_bytes(C.byref(_desc(width, param_width, _abi.RSN_MMA_F32, layers, skip)))
        split = lib.rsn_packed_weights_bytes(C.byref(_desc(width, param_width, _abi.RSN_MMA_BF16X3, layers, skip)))
        folded = lib.rsn_packed_weights_bytes(C.byref(_desc(width, param_width, _abi.RSN_MMA_F32_FOLDED, layers, skip)))
        assert plain > 0 and plain == split and folded > plain
        nb = width // 32
        assert plain >= 4 * (layers - 1) * 2 * 3 * (nb * 2) * nb * 256  # the split copies of the trunk alone, forward and transposed


def bf16_rne(x):
    """float32 array -> the nearest bf16 (ties to even) as float32: bf16 is the upper half of the float32 bit pattern."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def split3(x):
    """What split_elem (rsn_pack.hip) stores: round to nearest three times, each residual formed in float32."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    r1 = x - hi
    mid = bf16_rne(r1)
    r2 = r1 - mid
    lo = bf16_rne(r2)
    return hi, mid, lo


def _exact(x):
    hi, mid, lo = split3(x)
    return (hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)) == np.asarray(x, dtype=np.float32).astype(np.float64)


def test_three_bf16_pieces_add_up_to_the_fp32_value():
    rng = np.random.default_rng(7)
    # 10^6 values over the range the split covers, both signs: exponents -80 .. 100 times a factor kept above 2^-20
    m = rng.standard_normal(1_000_000)
    m = np.where(np.abs(m) < 1e-6, 1.0, m)
    x = (m * np.exp2(rng.integers(-80, 101, 1_000_000))).astype(np.float32)
    assert bool(_exact(x).all())
    weights = (rng.standard_normal(1_000_000) * 0.1).astype(np.float32)  # the magnitudes weights have
    assert bool(_exact(weights).all())
    e = np.arange(-108, 120)
    powers = np.exp2(e.astype(np.float64)).astype(np.float32)
    ones = (np.float32(2.0) - np.float32(2.0 ** -23)) * powers  # all-ones mantissas: every rounding carries
    picked = np.concatenate([powers, -powers, ones, -ones, np.zeros(2, np.float32), np.array([-0.0, 1.0, -1.0, 3.0, 255.0, 257.0], np.float32)])
    assert bool(_exact(picked).all())
    for p in split3(picked):  # each piece is a bf16: the low 16 bits are clear
        assert not bool((p.view(np.uint32) & 0xFFFF).any())


def test_the_split_loses_bits_only_below_the_underflow_limit():
    """bf16 has fp32's exponent range and 7 fraction bits: its smallest (subnormal) value is 2^-133, so the last piece of a value
    whose ulp 2^(e-23) lies below that is cut -- |x| < 2^-110.  Full 24-bit values on both sides of the limit."""
    full = np.float32(1.0) + np.float32(2.0 ** -23)  # lowest bit set: the third piece carries it
    at = np.array([full * np.float32(2.0 ** -110), -full * np.float32(2.0 ** -110), full * np.float32(2.0 ** -109)], np.float32)
    assert bool(_exact(at).all())
    below = np.array([full * np.float32(2.0 ** -111), full * np.float32(2.0 ** -112), -full * np.float32(2.0 ** -120)], np.float32)
    assert not bool(_exact(below).any())
    hi, mid, lo = split3(below)  # ... and what is lost is below one ulp of the value
    err = np.abs(hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64) - below.astype(np.float64))
    assert bool((err <= np.abs(below.astype(np.float64)) * 2.0 ** -23).all())
