"""CPU-side checks of the multi-scale data path: the numpy restatement of the pyramid is sound on its own, the level draw is
balanced, the parser and the run settings carry `multiscale`, and sizes and level counts that cannot work raise on the host."""
import math
import os
import re

import numpy as np
import pytest

from reflect_sampling_nerf_amd import _abi, _build, trainer
from reflect_sampling_nerf_amd.data import MAX_LEVELS, BlenderScene, RayDataManager, pyramid_layout
from tests.pyramid_reference import (pyramid_flat, pyramid_level, pyramid_level_float64, pyramid_offsets,
                                     sample_levels_and_indices)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(n=3, h=48, w=80, seed=0):
    """uint8 RGBA noise with one block of alpha 0 and one of alpha 255: both ends of the blend."""
    ims = np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 4), dtype=np.uint8)
    ims[0, :16, :32, 3] = 0
    ims[1, 16:48, 32:64, 3] = 255
    return ims


def test_reference_constant_image_stays_constant_with_equal_bits():
    for rgba in ((200, 13, 77, 255), (200, 13, 77, 91), (0, 0, 0, 255), (255, 255, 255, 3)):
        ims = np.broadcast_to(np.array(rgba, np.uint8), (2, 32, 48, 4)).copy()
        c, a = np.array(rgba[:3], np.int64), rgba[3]
        want = ((c * a + 255 * (255 - a)).astype(np.float32) / np.float32(65025)).view(np.uint32)  # S / 65025 of one pixel
        for level in range(1, 5):
            got = pyramid_level(ims, level)
            assert got.shape == (2, 32 >> level, 48 >> level, 3)
            # 4^l S / (65025 4^l): the same quotient, a power of two taken out of both exact operands
            assert np.array_equal(got.view(np.uint32), np.broadcast_to(want, got.shape)), (rgba, level)


def test_reference_alpha_zero_is_exactly_one():
    ims = np.random.default_rng(1).integers(0, 256, size=(2, 32, 32, 4), dtype=np.uint8)
    ims[..., 3] = 0
    for level in range(1, 5):
        assert np.array_equal(pyramid_level(ims, level), np.ones((2, 32 >> level, 32 >> level, 3), np.float32))


def test_reference_is_the_rounded_float64_box_average():
    ims = _images()
    for level in range(1, 5):
        want = pyramid_level_float64(ims, level).astype(np.float32)
        assert np.array_equal(pyramid_level(ims, level).view(np.uint32), want.view(np.uint32)), level


def test_layout_matches_the_restatement_and_the_header():
    sizes, off = pyramid_layout(3, 48, 80, 5)
    assert sizes == ((48, 80), (24, 40), (12, 20), (6, 10), (3, 5))
    assert list(off) == pyramid_offsets(3, 48, 80, 5) == [0, 0, 2880, 3600, 3780, 3825]
    assert pyramid_flat(_images(), 5).shape == (3825, 3)
    assert pyramid_layout(7, 37, 53, 1) == (((37, 53),), (0, 0))  # one level: any size, an empty allocation
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(rf"#define RSN_PYRAMID_MAX_LEVELS {MAX_LEVELS}\b", header) and MAX_LEVELS == 5
    assert "rsn_pyramid.hip" in _build.SOURCES
    assert {"rsn_build_pyramid", "rsn_sample_pyramid_rays"} <= set(_abi.EXPORTED_SYMBOLS)


@pytest.mark.parametrize("levels,worst_recorded", [(3, 2.92), (4, 2.30), (5, 2.58)])
def test_level_draw_is_balanced_in_the_restatement(levels, worst_recorded):
    """R = 65536 rays of (seed 3, rank 0, step 7): every level's count within 4 sigma of R / L, sigma = sqrt(R (1/L)(1 - 1/L)) (a
    binomial count); the worst level lies at the recorded number of sigmas.  Every index lies inside its level's image."""
    R = 65536
    lvl, idx = sample_levels_and_indices(3, 48, 80, levels, R, seed=3, rank=0, step=7)
    counts = np.bincount(lvl, minlength=levels)
    assert counts.shape == (levels,) and counts.sum() == R
    sigma = math.sqrt(R * (1.0 / levels) * (1.0 - 1.0 / levels))
    dev = np.abs(counts - R / levels) / sigma
    assert dev.max() <= 4.0, dev
    assert round(float(dev.max()), 2) == worst_recorded, dev
    assert (idx >= 0).all() and (idx[:, 0] < 3).all() and (idx[:, 1] < (48 >> lvl)).all() and (idx[:, 2] < (80 >> lvl)).all()


def test_one_level_draws_the_single_scale_pixels():
    from tests.data_reference import sample_indices

    lvl, idx = sample_levels_and_indices(5, 37, 53, 1, 4096, seed=1234, rank=2, step=17)
    assert not lvl.any() and np.array_equal(idx, sample_indices(5, 37, 53, 4096, seed=1234, rank=2, step=17))


def test_parser_accepts_multiscale():
    for ap, absent in ((trainer.build_parser(), 1), (trainer.build_parser(run_defaults=False), None)):
        assert ap.parse_args(["train", "--data", "D", "--out", "O"]).multiscale == absent
        assert ap.parse_args(["train", "--data", "D", "--out", "O", "--multiscale", "4"]).multiscale == 4
        assert ap.parse_args(["eval", "--data", "D", "--ckpt", "C"]).multiscale == 1
        assert ap.parse_args(["eval", "--data", "D", "--ckpt", "C", "--multiscale", "3"]).multiscale == 3
    for argv in (["train", "--data", "D", "--out", "O", "--multiscale", "6"], ["eval", "--data", "D", "--ckpt", "C", "--multiscale", "0"]):
        with pytest.raises(SystemExit):  # refused on the command line, before a GPU or a file is looked for
            trainer.main(argv)


def test_run_state_and_settings_carry_multiscale_only_above_one():
    keys = {"version", "seed", "rays", "mma", "deterministic", "cuda_rng_state", "cpu_rng_state"}
    assert set(trainer.make_run_state(0, 8, "f32", False, "cpu")) == keys
    assert set(trainer.make_run_state(0, 8, "f32", False, "cpu", multiscale=1)) == keys
    rs = trainer.make_run_state(0, 8, "f32", False, "cpu", multiscale=3)
    assert set(rs) == keys | {"multiscale"} and rs["multiscale"] == 3
    none = dict.fromkeys(("rays", "mma", "seed", "deterministic", "max_grad_norm", "skip_nonfinite", "multiscale"))
    fresh, notes = trainer._resolve_run_settings(none, None)
    assert (fresh["multiscale"], notes) == (1, [])
    got, notes = trainer._resolve_run_settings(none, rs)  # --resume without restating it
    assert (got["multiscale"], notes) == (3, [])
    got, notes = trainer._resolve_run_settings({**none, "multiscale": 2}, rs)  # a given value wins and says so
    assert got["multiscale"] == 2 and len(notes) == 1 and "multiscale" in notes[0] and "not bit-exact" in notes[0]
    plain = trainer.make_run_state(0, 8, "f32", False, "cpu")
    assert trainer._resolve_run_settings(none, plain)[0]["multiscale"] == 1  # a single-scale checkpoint resumes single-scale


def _scene(h, w, n=2):
    return BlenderScene.from_arrays(np.zeros((n, h, w, 4), np.uint8), np.tile(np.eye(4, dtype=np.float32)[:3], (n, 1, 1)), focal=50.0)


def test_indivisible_size_raises_before_any_device_call():
    """48 x 80 carries five levels, 48 x 40 four (40 / 16 is no integer), 37 x 53 one.  The data manager checks before it uploads
    anything (the device named here does not exist), the trainer before it builds a model, eval before it reads the checkpoint."""
    pyramid_layout(3, 48, 80, 5)
    for h, w, levels in ((48, 40, 5), (37, 53, 2), (50, 80, 3)):
        with pytest.raises(ValueError, match="divisible"):
            pyramid_layout(3, h, w, levels)
        with pytest.raises(ValueError, match="divisible"):
            RayDataManager(_scene(h, w), "no-such-device", levels=levels)
        with pytest.raises(ValueError, match="divisible"):
            trainer.train(_scene(h, w), "unused", steps=2, device="no-such-device", log=None, multiscale=levels)
        with pytest.raises(ValueError, match="divisible"):
            trainer.evaluate(_scene(h, w), "no-such-checkpoint", device="no-such-device", multiscale=levels)
    assert not os.path.exists("unused")


@pytest.mark.parametrize("levels", [0, 6, -1])
def test_level_count_out_of_range_raises(levels):
    with pytest.raises(ValueError, match="1 to 5"):
        pyramid_layout(3, 64, 64, levels)
    with pytest.raises(ValueError, match="1 to 5"):
        RayDataManager(_scene(64, 64), "no-such-device", levels=levels)
    with pytest.raises(ValueError, match="1 to 5"):
        trainer.evaluate(_scene(64, 64), "no-such-checkpoint", device="no-such-device", multiscale=levels)


def test_eval_names_a_level_too_small_for_ssim():
    with pytest.raises(ValueError, match=r"level 2 are 10 x 12 pixels.*11 x 11"):
        trainer.evaluate(_scene(48, 40), "no-such-checkpoint", device="no-such-device", multiscale=3)
    assert trainer.eval_level_sizes(_scene(48, 48), 3) == ((48, 48), (24, 24), (12, 12))


def test_c_calls_refuse_bad_arguments_without_a_device():
    """The argument checks of both C calls come before any launch, so they answer on a machine without a GPU too; the full matrix of
    message fragments is in test_pyramid_gpu.py."""
    _build.build_library()
    lib = _abi.load_library()
    assert lib.rsn_build_pyramid(3, 48, 80, 6, None, None, 0, None) == -1 and b"levels=6" in lib.rsn_last_error()
    assert lib.rsn_build_pyramid(3, 48, 40, 5, None, None, 0, None) == -1 and b"divisible by 2^(levels-1) = 16" in lib.rsn_last_error()
    assert lib.rsn_build_pyramid(3, 37, 53, 1, None, None, 0, None) == 0  # one level: nothing to build, no pointer read
    assert lib.rsn_sample_pyramid_rays(3, 48, 80, 0, None, None, 0, None, 1.0, 1.0, 0.0, 0.0, 4, 0, 0, 0, None, None, None, None, None,
                                       None, None) == -1 and b"levels=0" in lib.rsn_last_error()
