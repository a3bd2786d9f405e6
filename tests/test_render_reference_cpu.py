"""The float64 references of tests/render_reference.py, checked on the host alone: the compositing gradients from autograd through
oracle/cpu_ref.py against the closed form of the kernel source's header comment (coded independently), and the exclusion caps of
tests/test_render_ops_gpu.py evaluated on the reference for every seed and shape that file uses."""
import numpy as np
import pytest
import torch

from tests import render_reference as rr


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("background", [0, 1, 2])
@pytest.mark.parametrize("S", [1, 5, 130])
def test_composite_autograd_reference_equals_closed_form(S, background, clip):
    """dL/dx_k = g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i against fp64 autograd, to 1e-12 (of the ray's largest entry, at least 1)."""
    inp = rr.composite_inputs(rr.COMPOSITE_R, S, rr.composite_seed(S, background))
    ref, _, _ = rr.composite_reference(inp, background, False, clip)
    closed = rr.composite_closed_form(inp, background, clip)
    err = (ref["g_sigma"] - closed).abs().amax(-1) / closed.abs().amax(-1).clamp(min=1.0)
    print(f"S={S} background={background} clip={clip}: worst {float(err.max()):.3e}")
    assert float(err.max()) <= 1e-12
    assert float(closed.abs().max()) > 1e-3  # the comparison is not between zeros


def test_planted_clip_rays_sit_exactly_on_the_bounds():
    """Ray 3 composites to exactly 1.0 and ray 4 to exactly 0.0 in fp64 (the GPU test requires their gradients to pass the clip)."""
    for S in rr.COMPOSITE_S:
        for background in (0, 1, 2):
            inp = rr.composite_inputs(rr.COMPOSITE_R, S, rr.composite_seed(S, background))
            ref, _, _ = rr.composite_reference(inp, background, False, True)
            assert bool((ref["unclipped"][3] == 1.0).all()), (S, background)
            if background != 1:
                assert bool((ref["unclipped"][4] == 0.0).all()), (S, background)
                assert float(ref["g_color"][4].abs().max()) > 0 or float(ref["weights"][4].max()) == 0
            assert float(ref["g_color"][3, 0].min()) > 0.2  # the gradient passes at equality


def _composite_cases():
    for S in rr.COMPOSITE_S:
        for background in (0, 1, 2):
            yield rr.COMPOSITE_R, S, rr.composite_seed(S, background), background
    for background in (0, 1, 2):
        yield rr.BIG_R, rr.BIG_S, rr.composite_seed(rr.BIG_S, background) + 1, background


def test_clip_exclusion_cap_holds_for_every_compositing_case():
    for R, S, seed, background in _composite_cases():
        inp = rr.composite_inputs(R, S, seed)
        ref, _, _ = rr.composite_reference(inp, background, False, True)
        n = int(ref["clip_near"].sum())
        clipped = int(((ref["unclipped"] < 0) | (ref["unclipped"] > 1)).any(-1).sum())
        print(f"R={R} S={S} background={background}: {n} rays within {rr.CLIP_EXCLUDE} of a clip bound, {clipped} rays clip")
        assert n <= rr.CLIP_CAP * R
        assert not bool(ref["clip_near"][:rr.PLANTED].any())
        if S > 1:
            assert clipped >= 0.1 * R, "a good share of rays must clip decisively"


@pytest.mark.parametrize("R", rr.REFLECT_R)
@pytest.mark.parametrize("pattern", rr.REFLECT_PATTERNS)
def test_reflect_mask_exclusion_cap_and_patterns(R, pattern):
    inp, planted = rr.reflect_inputs(R, pattern, rr.reflect_seed(R, pattern))
    ref, near = rr.reflect_reference(inp, planted, 4.0)
    M = int(ref["mask"].sum())
    print(f"R={R} {pattern}: M={M}, {int(near.sum())} rays within {rr.MASK_EXCLUDE} of a threshold")
    assert int(near.sum()) <= rr.MASK_CAP * R
    if pattern == "none":
        assert M == 0
    if pattern == "all":
        assert M == R
    if pattern == "random" and R > 1000:
        assert 0.35 * R <= M <= 0.45 * R
    if pattern == "last" and R > 1024:
        first = ((R - 1) // 1024) * 1024
        assert M > 0 and not bool(ref["mask"][:first].any())
    if planted:
        a, b, c, d = planted
        assert not bool(ref["mask"][a]) and bool(ref["mask"][b]) and not bool(ref["mask"][c]) and bool(ref["mask"][d])
        assert float(ref["n_dot_d"][c]) == 0.0 and float(ref["n_dot_d"][d]) == -2.0 ** -20
        assert inp["accumulation"][a].item() == float(rr.ACC_THRESHOLD)
        assert np.float32(inp["accumulation"][b].item()) == np.nextafter(rr.ACC_THRESHOLD, np.float32(1))
    # the relative bounds of the GPU test rely on inputs that do not cancel
    nd = inp["pred_normals"].double() * inp["directions"].double()
    assert bool(((nd >= 0).all(-1) | (nd <= 0).all(-1)).all())
    od = inp["origins"].double() * inp["directions"].double()
    assert bool((od >= 0).all())


@pytest.mark.parametrize("R", [1025, 3001])
def test_combine_clip_exclusion_cap_and_planted_bounds(R):
    idx = torch.arange(3, R, 2)  # any compaction: the planted elements sit on its first two rays
    ci = rr.combine_inputs(R, 7000 + R, idx)
    ref = rr.combine_reference(ci, idx)
    assert int(ref["near"].sum()) <= rr.CLIP_CAP * R
    assert ref["v"][0].tolist() == [1.0, 0.0, 0.0] and ref["v"][1].tolist() == [1.0, 1.0, 1.0]
    assert float(ref["g_comp"][:2].min()) > 0  # the gradient passes at equality
    v = ref["v"]
    for lo, hi in ((None, -1e-3), (1e-3, 1 - 1e-3), (1 + 1e-3, None)):
        m = torch.ones_like(v, dtype=torch.bool)
        if lo is not None:
            m &= v > lo
        if hi is not None:
            m &= v < hi
        assert int(m.sum()) > 0.1 * v.numel()  # decisive values on every side
