"""CPU checks of per-sample empty-space skipping: the three calls in the header, the binding and the library (ABI 18 still), the
refusals of the host-only workspace function, the command line, and the fp64 reference (tests/occupancy_samples_reference.py)
against a brute-force point sampling of the sub-segments."""
import os
import re

import numpy as np
import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import occupancy_reference as ref
from tests import occupancy_samples_reference as sref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("rsn_occupancy_samples_workspace_bytes", "rsn_occupancy_compact_samples", "rsn_scatter_level")


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def test_the_three_calls_are_declared_bound_and_exported_at_abi_18(lib):
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(r"#define RSN_ABI_VERSION 18\b", header) and _abi.RSN_ABI_VERSION == 18 and lib.rsn_abi_version() == 18
    for name in NEW_CALLS:
        assert re.search(rf"\b(size_t|int) {name}\(", header), name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    for rule in ("max_radius", "sample_index", "n_live", "never read", "left unwritten", "written as zeros"):
        assert rule in header, rule


def test_workspace_function_refuses_what_the_header_says(lib):
    ws = lib.rsn_occupancy_samples_workspace_bytes
    assert ws(0, 1) > 0 and ws(1, 1) > 0
    assert ws(4096, 128) >= 4 * (4096 * 128 // 256 + 1)
    for bad in ((-1, 4), (4, 0), (4, -3)):
        assert ws(*bad) == 0 and b"n_rays" in lib.rsn_last_error(), bad
    # n_rays * n_samples * 3 has to fit in int32: 2^31 - 1 = 3 * 715827882 + 1
    assert ws(715827882, 1) > 0 and ws(715827883, 1) == 0
    assert ws(5592405, 128) > 0 and ws(5592406, 128) == 0  # 3 * 128 * 5592405 = 2^31 - 128
    assert ws(2 ** 31 - 1, 2 ** 31 - 1) == 0


def test_the_commands_accept_skip_empty_samples():
    ap = trainer.build_parser()
    for cmd in (["render", "--ckpt", "c", "--out", "o"], ["eval", "--data", "d", "--ckpt", "c"]):
        plain = ap.parse_args(cmd)
        assert plain.skip_empty_samples is False and trainer.resolve_occupancy_args(ap, plain) is None
        parent = {"resolution": 128, "sigma": 0.01, "dilate": 1, "bounds": None}  # what --skip-empty alone has always resolved to
        rays_only = trainer.resolve_occupancy_args(ap, ap.parse_args(cmd + ["--skip-empty"]))
        # The switch is off there.  The key is absent rather than False: tests/test_occupancy_cpu.py, which is not to be edited,
        # compares this dict with the parent's for equality; every reader takes the absent key as False.
        assert rays_only == parent and rays_only.get("samples", False) is False
        assert {**rays_only, "samples": rays_only.get("samples", False)} == {**parent, "samples": False}
        for flags in (["--skip-empty-samples"], ["--skip-empty", "--skip-empty-samples"]):  # alone it turns both switches on
            on = trainer.resolve_occupancy_args(ap, ap.parse_args(cmd + flags))
            assert on == {**parent, "samples": True}
        full = trainer.resolve_occupancy_args(ap, ap.parse_args(cmd + [
            "--skip-empty-samples", "--occupancy-resolution", "96", "--occupancy-sigma", "0.5", "--occupancy-dilate", "2",
            "--occupancy-bounds", "-3", "-3", "-3", "3", "3", "3.5"]))
        assert full == {"resolution": 96, "sigma": 0.5, "dilate": 2, "bounds": (-3.0, -3.0, -3.0, 3.0, 3.0, 3.5), "samples": True}
        with pytest.raises(SystemExit):
            trainer.resolve_occupancy_args(ap, ap.parse_args(cmd + ["--skip-empty-samples", "--occupancy-resolution", "1"]))
    with pytest.raises(SystemExit):  # training never uses it
        ap.parse_args(["train", "--data", "d", "--out", "o", "--skip-empty-samples"])


def test_help_calls_the_margin_a_design_rule(capsys):
    ap = trainer.build_parser()
    with pytest.raises(SystemExit):
        ap.parse_args(["render", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--skip-empty-samples" in text and "implies --skip-empty" in text and "design rule" in text


def test_reference_marks_sub_segments_and_agrees_with_point_sampling():
    """On DIMS[1], per sub-segment: the reference's predicates are hits_shrunk / hits_grown of the sub-segment; a sampled point in
    an occupied cell implies `may`; and a sub-segment that meets a cell shrunk by DELTA = 0.05 of a cell contains a point q at
    least DELTA * min(spacing) from every face of the cell, hence a run of that length inside the cell or an end point in it, so
    with a point spacing below that length a sampled point lies in the cell."""
    dims, gi, K, DELTA = ref.DIMS[1], 1, 4096, 0.05
    origin, spacing = ref.grid_frame(dims, gi)
    checked = 0
    for si, share in enumerate((0.05, 0.5)):
        occ = ref.grid_case(dims, share, 2 * gi + si)
        for S in (1, 4):
            o, d, near, far, fam = ref.ray_cases(dims, origin, spacing, 140, 50 + 10 * si + S)
            bins = sref.make_bins(near, far, S, S + si)
            assert bins.shape == (140, S + 1) and bins.dtype == np.float32
            oo, dd, t0, t1 = sref.expand(o, d, bins)
            assert np.array_equal(oo[S - 1], o[0]) and np.array_equal(t1[:S], bins[0, 1:]) and len(t0) == 140 * S
            for outside in (False, True):
                must, may, bad = sref.sample_predicates(o, d, bins, occ, origin, spacing, outside)
                assert np.array_equal(must, ref.hits_shrunk(oo, dd, t0, t1, occ, origin, spacing, outside))
                assert np.array_equal(may, ref.hits_grown(oo, dd, t0, t1, occ, origin, spacing, outside))
                assert not (must & ~may).any() and must[bad].all() and bad.any() and not bad.all()
                ok = ~bad
                sub = np.flatnonzero(ok)
                o_ok = np.where(bad[:, None], 0.0, oo).astype(np.float32)  # brute_force wants finite numbers: masked out below
                d_ok = np.where(bad[:, None], 0.0, dd).astype(np.float32)
                b_ok = np.where(bad[:, None], 0.0, np.stack([t0, t1], axis=1)).astype(np.float32)
                brute = sref.brute_force(o_ok, d_ok, b_ok, occ, origin, spacing, outside, K)
                assert not (brute & ~may)[sub].any()
                strong = ref._predicate(oo, dd, t0, t1, occ, origin, spacing, outside, DELTA)
                with np.errstate(invalid="ignore"):
                    length = (t1.astype(np.float64) - t0) * np.linalg.norm(dd.astype(np.float64), axis=1)
                    dense = ok & (length / K < DELTA * float(spacing.min()))
                assert dense.sum() >= 0.8 * ok.sum()
                missed = np.flatnonzero(dense & strong & ~brute)
                assert len(missed) == 0, (share, S, outside, missed[:5])
                assert (strong & dense).any() and (~may & dense).any()  # both answers occur
                checked += int(dense.sum())
    assert checked >= 2000
    # the footprint rule by hand: |d| = 2, pixel_area = pi * 0.01 -> radius 0.1 * 2 * t
    fp = sref.footprint(np.float32([[0, 0, 2]]), np.float32([np.pi * 0.01]), np.float32([[0, 1, 2, 3]]), 0.5)
    assert fp.tolist() == [[False, False, True]]
    assert sref.footprint(np.float32([[0, 0, 2]]), np.float32([np.nan]), np.float32([[0, 1]]), np.inf).tolist() == [[True]]
    assert sref.footprint(np.float32([[0, 0, 2]]), np.float32([1.0]), np.float32([[0, 1e30]]), np.inf).tolist() == [[False]]
