"""Geometry metrics (eval --normals), everything that needs no GPU: the normal-map loader, the float64 reference against its own
definition and against the literal multinerf formula, the ABI and CLI surface, and the argument checks of rsn_normal_error (which
come before any launch)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from reflect_sampling_nerf_amd import _abi, _build, trainer
from reflect_sampling_nerf_amd.data import BlenderScene, load_blender_split
from tests import geometry_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ loader
def _write_scene(root, n=3, H=6, W=5, suffix="_normal", normal_mode="RGB", seed=0):
    from PIL import Image

    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "test"), exist_ok=True)
    images = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8)
    normals = rng.integers(0, 256, size=(n, H, W, 4 if normal_mode == "RGBA" else 3), dtype=np.uint8)
    frames = []
    for i in range(n):
        Image.fromarray(images[i], "RGBA").save(os.path.join(root, "test", f"r_{i}.png"))
        Image.fromarray(normals[i], normal_mode).save(os.path.join(root, "test", f"r_{i}{suffix}.png"))
        pose = np.eye(4)
        pose[:3, 3] = rng.standard_normal(3)
        frames.append({"file_path": f"./test/r_{i}", "transform_matrix": pose.tolist()})
    with open(os.path.join(root, "transforms_test.json"), "w") as fh:
        json.dump({"camera_angle_x": 0.69, "frames": frames}, fh)
    return images, normals[..., :3]


@pytest.mark.parametrize("mode", ["RGB", "RGBA"])
def test_loader_round_trips_normal_maps_byte_for_byte(tmp_path, mode):
    images, normals = _write_scene(str(tmp_path), normal_mode=mode)  # RGBA: the normal file's own alpha channel is ignored
    with_n = load_blender_split(str(tmp_path), "test", normals=True)
    assert with_n.normals.dtype == np.uint8 and with_n.normals.shape == (3, 6, 5, 3)
    assert np.array_equal(with_n.normals, normals) and np.array_equal(with_n.images, images)
    without = load_blender_split(str(tmp_path), "test")
    assert without.normals is None
    assert np.array_equal(without.images, with_n.images) and np.array_equal(without.c2w, with_n.c2w)
    assert (without.fx, without.fy, without.cx, without.cy) == (with_n.fx, with_n.fy, with_n.cx, with_n.cy)


def test_loader_custom_suffix_missing_file_and_size_mismatch(tmp_path):
    from PIL import Image

    _, normals = _write_scene(str(tmp_path), suffix="_nrm")
    assert np.array_equal(load_blender_split(str(tmp_path), "test", normals=True, normals_suffix="_nrm").normals, normals)
    with pytest.raises(FileNotFoundError, match=r"r_0_normal\.png.*frame 0"):  # the default suffix names files that are not there
        load_blender_split(str(tmp_path), "test", normals=True)
    os.remove(tmp_path / "test" / "r_1_nrm.png")
    with pytest.raises(FileNotFoundError, match=r"r_1_nrm\.png.*frame 1"):
        load_blender_split(str(tmp_path), "test", normals=True, normals_suffix="_nrm")
    Image.fromarray(np.zeros((4, 7, 3), np.uint8), "RGB").save(tmp_path / "test" / "r_1_nrm.png")
    with pytest.raises(ValueError, match=r"7 x 4.*5 x 6"):
        load_blender_split(str(tmp_path), "test", normals=True, normals_suffix="_nrm")
    assert load_blender_split(str(tmp_path), "test").normals is None  # the broken map is not opened when it is not asked for


def test_from_arrays_encodes_unit_normals_within_the_quantisation_bound():
    """rint((n/2 + 1/2) 255) is off by at most 1/2, so every component of the decoded vector (2u - 255) / 255 is within 1/255 of n's,
    the decoded vector within sqrt(3)/255 of the unit vector n, and the angle between them within sqrt(3)/255 rad = 0.389 degrees."""
    rng = np.random.default_rng(5)
    n = rng.standard_normal((1000, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    maps = n.reshape(1, 25, 40, 3)
    pose = np.eye(4, dtype=np.float32)[None, :3]
    sc = BlenderScene.from_arrays(np.zeros((1, 25, 40, 3), np.uint8), pose, focal=30.0, normals=maps)
    assert sc.normals.dtype == np.uint8 and sc.normals.shape == (1, 25, 40, 3)
    dec = ref.decode(sc.normals).reshape(-1, 3) / 255.0
    assert np.abs(dec - n).max() <= 1.0 / 255.0 + 1e-12
    bound_deg = math.degrees(math.sqrt(3.0) / 255.0)
    worst = ref.angle_deg(n, dec).max()
    print(f"quantisation: worst angle {worst:.4f} deg, bound {bound_deg:.4f} deg")
    assert worst <= bound_deg
    as_bytes = sc.normals.copy()
    assert np.array_equal(BlenderScene.from_arrays(np.zeros((1, 25, 40, 3), np.uint8), pose, focal=30.0, normals=as_bytes).normals, as_bytes)
    assert BlenderScene.from_arrays(np.zeros((1, 25, 40, 3), np.uint8), pose, focal=30.0).normals is None
    for bad in (np.zeros((1, 25, 40, 4)), np.zeros((1, 25, 41, 3)), np.zeros((25, 40, 3)), np.zeros((2, 25, 40, 3), np.uint8)):
        with pytest.raises(ValueError, match="normals must be"):
            BlenderScene.from_arrays(np.zeros((1, 25, 40, 3), np.uint8), pose, focal=30.0, normals=bad)


# ------------------------------------------------------------------------------------------------ the reference, in float64
def _one(p, u, a=255, acc=None, rotation=None):
    p, u = np.atleast_2d(np.asarray(p, dtype=np.float64)), np.atleast_2d(np.asarray(u, dtype=np.uint8))
    rgba = np.zeros((len(u), 4), np.uint8)
    rgba[:, 3] = a
    return ref.normal_error(p, acc, u, rgba, rotation)


def test_reference_angles_of_known_pairs():
    u = np.array([200, 90, 30], np.uint8)
    g = ref.decode(u)
    ortho = np.cross(g, [0.0, 0.0, 1.0])
    for p, want in ((g, 0.0), (-g, 180.0), (ortho, 90.0), (np.zeros(3), 90.0)):
        for scale in (1.0, 1e-3, 1e3):
            got = _one(p * scale, u)
            assert got["out"][0] == pytest.approx(want, abs=1e-9) and got["out"][3] == 1.0 and got["out"][1] == 1.0
    rng = np.random.default_rng(1)
    p = rng.standard_normal((50, 3))
    gt = rng.integers(0, 256, size=(50, 3), dtype=np.uint8)
    base = _one(p, gt)["error_map"]
    for scale in (1e-3, 1e3):
        assert np.abs(_one(p * scale, gt)["error_map"] - base).max() <= 1e-9


def test_reference_excludes_neutral_normals_and_zero_alpha_and_weights_by_alpha():
    good = np.array([200, 90, 30], np.uint8)
    for neutral in ((127, 127, 127), (128, 128, 128), (127, 128, 127), (128, 127, 128)):
        r = _one([1.0, 0.0, 0.0], neutral)
        assert not r["valid"][0] and r["error_map"][0] == 0.0 and math.isnan(r["out"][0]) and r["out"][1] == 0.0 and r["out"][3] == 0.0
    assert _one([1.0, 0.0, 0.0], (126, 128, 128))["valid"][0] and _one([1.0, 0.0, 0.0], (128, 129, 128))["valid"][0]
    r = _one([1.0, 0.0, 0.0], good, a=0)
    assert not r["valid"][0] and math.isnan(r["out"][0]) and r["out"][1] == 0.0
    # alphas 255 and 51: the 5 : 1 weighted mean of 0 and 180 degrees is 30
    g = ref.decode(good)
    r = _one(np.stack([g, -g]), np.stack([good, good]), a=np.array([255, 51], np.uint8))
    assert r["out"][0] == pytest.approx((5.0 * 0.0 + 1.0 * 180.0) / 6.0, abs=1e-9)
    assert r["out"][1] == pytest.approx(306.0 / 255.0, abs=1e-12) and r["out"][3] == 2.0
    # alpha error: over ALL pixels, valid or not
    r = _one(np.stack([g, g, g]), np.stack([good, good, (128, 128, 128)]), a=np.array([255, 0, 51], np.uint8), acc=np.array([0.75, 0.5, 0.0]))
    assert r["out"][2] == pytest.approx((0.25 + 0.5 + 0.2) / 3.0, abs=1e-12)
    assert _one(g, good)["out"][2] == 0.0  # no accumulation given


def test_reference_rotation_equals_rotating_the_decoded_vectors_by_hand():
    rng = np.random.default_rng(2)
    p = rng.standard_normal((40, 3))
    gt = rng.integers(0, 256, size=(40, 3), dtype=np.uint8)
    c2w = np.concatenate([ref.rotation_matrix(), np.array([[1.0], [2.0], [3.0]], np.float32)], axis=1)
    R = c2w[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and np.abs(R - np.eye(3)).max() > 0.5
    by_hand = np.stack([ref.angle_deg(p[i], R @ ref.decode(gt[i])) for i in range(40)])
    got = _one(p, gt, rotation=c2w[:3, :3])
    assert np.abs(got["error_map"] - np.where(got["valid"], by_hand, 0.0)).max() <= 1e-9
    assert np.abs(got["error_map"] - _one(p, gt)["error_map"]).max() > 1.0  # the rotation matters


def test_reference_agrees_with_the_literal_multinerf_formula():
    """arccos(clip(<l2n(p), l2n(g)>)) in float64 on random pairs whose angle lies in [1, 179] degrees, where arccos is accurate."""
    rng = np.random.default_rng(3)
    p = rng.standard_normal((20000, 3)) * np.exp(rng.uniform(-4, 1, size=(20000, 1)))
    gt = rng.integers(0, 256, size=(20000, 3), dtype=np.uint8)
    g = ref.decode(gt)
    mine = ref.angle_deg(p, g)
    keep = (mine >= 1.0) & (mine <= 179.0) & ref.valid_mask(gt, np.full(20000, 255))
    assert keep.sum() > 15000
    assert np.abs(mine[keep] - ref.multinerf_angle_deg(p[keep], g[keep])).max() <= 1e-9
    # and the alpha-weighted mean is multinerf's sum(w * angle) / sum(w)
    alpha = rng.choice(np.array(ref.ALPHAS, dtype=np.uint8), size=20000)
    rgba = np.zeros((20000, 4), np.uint8)
    rgba[:, 3] = alpha
    w = np.where(ref.valid_mask(gt, alpha), alpha / 255.0, 0.0)
    assert ref.normal_error(p, None, gt, rgba)["out"][0] == pytest.approx((w * mine).sum() / w.sum(), rel=1e-12)


# ------------------------------------------------------------------------------------------------ ABI and CLI
def test_symbols_source_and_abi_version():
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    for name in ("rsn_normal_error_workspace_bytes", "rsn_normal_error"):
        assert name + "(" in header and name in _abi.EXPORTED_SYMBOLS
    assert "rsn_geometry.hip" in _build.SOURCES and os.path.isfile(os.path.join(_build.CSRC, "rsn_geometry.hip"))
    assert _abi.RSN_ABI_VERSION == 18 and "#define RSN_ABI_VERSION 18" in header
    assert f"#define RSN_NORMAL_ERROR_MAX_GROUPS {_abi.RSN_NORMAL_ERROR_MAX_GROUPS}\n" in header
    assert _abi.RSN_NORMAL_ERROR_MAX_PIXELS == 1 << 24 and "#define RSN_NORMAL_ERROR_MAX_PIXELS (1 << 24)" in header


def test_eval_flags_parse_and_default_off():
    ap = trainer.build_parser()
    plain = ap.parse_args(["eval", "--data", "d", "--ckpt", "c"])
    assert plain.normals is False and plain.normals_suffix is None and plain.normals_space is None
    on = ap.parse_args(["eval", "--data", "d", "--ckpt", "c", "--normals", "--normals-suffix", "_n", "--normals-space", "camera"])
    assert on.normals is True and on.normals_suffix == "_n" and on.normals_space == "camera"
    assert trainer.DEFAULT_NORMALS_SUFFIX == "_normal" and trainer.NORMALS_SPACES == ("world", "camera")
    with pytest.raises(SystemExit):
        ap.parse_args(["eval", "--data", "d", "--ckpt", "c", "--normals", "--normals-space", "tangent"])
    with pytest.raises(SystemExit):
        ap.parse_args(["train", "--data", "d", "--out", "o", "--normals"])  # an eval flag


@pytest.mark.parametrize("flag", [["--normals-suffix", "_n"], ["--normals-space", "camera"], ["--normals-space", "world"]])
def test_dependent_flag_without_normals_is_an_argparse_error(flag, capsys):
    with pytest.raises(SystemExit) as e:
        trainer.main(["eval", "--data", "no-such-dir", "--ckpt", "no-such-checkpoint", *flag])
    assert e.value.code == 2
    assert f"{flag[0]} need(s) --normals" in capsys.readouterr().err


def test_evaluate_refuses_a_scene_without_normals_before_checkpoint_and_device():
    sc = BlenderScene.from_arrays(np.zeros((2, 48, 48, 4), np.uint8), np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1)), focal=50.0)
    with pytest.raises(ValueError, match="scene.normals is None"):
        trainer.evaluate(sc, "no-such-checkpoint", device="no-such-device", normals=True)
    with pytest.raises(ValueError, match="scene.normals is None"):
        trainer.evaluate(sc, "no-such-checkpoint", device="no-such-device", normals=True, multiscale=2)
    with_n = BlenderScene.from_arrays(np.zeros((2, 48, 48, 4), np.uint8), np.tile(np.eye(4, dtype=np.float32)[:3], (2, 1, 1)), focal=50.0,
                                      normals=np.zeros((2, 48, 48, 3), np.uint8))
    with pytest.raises(ValueError, match="normals_space"):
        trainer.evaluate(with_n, "no-such-checkpoint", device="no-such-device", normals=True, normals_space="tangent")
    with pytest.raises((RuntimeError, FileNotFoundError)):  # a sound request gets as far as the device and the checkpoint named here
        trainer.evaluate(with_n, "no-such-checkpoint", device="no-such-device", normals=True)


def test_c_call_refuses_bad_arguments_without_a_device():
    """The argument checks come before any launch, so they answer on a machine without a GPU; the pointers are never read."""
    _build.build_library()
    lib = _abi.load_library()
    p = C.c_void_p(4096)  # never dereferenced: every call below fails its checks first
    assert lib.rsn_normal_error_workspace_bytes(1) == 32 and lib.rsn_normal_error_workspace_bytes(257) == 64
    assert lib.rsn_normal_error_workspace_bytes(256 * 256 + 1) == 32 * 256 == lib.rsn_normal_error_workspace_bytes(1 << 24)
    assert lib.rsn_normal_error_workspace_bytes(0) == 0 and lib.rsn_normal_error_workspace_bytes((1 << 24) + 1) == 0
    for n in (0, -3, (1 << 24) + 1):
        assert lib.rsn_normal_error(n, p, p, p, p, p, p, p, 1 << 20, p, None) == -1 and f"n_pixels={n}".encode() in lib.rsn_last_error()
    for hole in (1, 3, 4, 7, 9):  # normals, gt_normals, gt_rgba, workspace, out
        args = [100, p, p, p, p, p, p, p, 1 << 20, p, None]
        args[hole] = None
        assert lib.rsn_normal_error(*args) == -1 and b"NULL" in lib.rsn_last_error()
    assert lib.rsn_normal_error(100, p, p, p, p, p, p, p, 31, p, None) == -4 and b"31 bytes, 32 needed" in lib.rsn_last_error()
    assert lib.rsn_normal_error(70000, p, p, p, p, p, p, p, 8191, p, None) == -4 and b"8192 needed" in lib.rsn_last_error()
    assert lib.rsn_normal_error(100, p, p, p, p, p, p, C.c_void_p(4100), 64, p, None) == -1 and b"aligned" in lib.rsn_last_error()
