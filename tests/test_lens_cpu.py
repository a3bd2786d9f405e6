"""CPU checks of the capture input side's opt-ins (masks, fisheye cameras, downscaled image sets): today's refusals with the opt-ins
off, the same captures loading with them on, the 12-column table, mask files of every mode, the images_K rule, the float64 fisheye
reference against itself and against the loader's invertibility check, the reference list rule, the parser and the checkpoint."""
import json
import math
import os

import numpy as np
import pytest

from reflect_sampling_nerf_amd import _abi, checkpoint, data, trainer
from tests import capture_reference as cref
from tests import lens_reference as ref

H, W = 36, 52
ON = dict(masks=True, fisheye=True)
RAW = dict(eval_mode="all", orientation="none", center="none", auto_scale=False)


def _images(n, seed=0, h=H, w=W):
    return np.random.default_rng(seed).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)


def _poses(n):
    rng = np.random.default_rng(1)
    return np.stack([cref.look_at(rng.normal(size=3) * 2.0 + np.array([0.0, 0.0, 3.0])) for _ in range(n)])


def _rows9(n):
    return np.stack([cref.camera_row(W, H, scale=1.0 + 0.01 * i) for i in range(n)])


def _old_capture(tmp_path, name, n=4, **kw):
    return cref.write_capture(str(tmp_path / name), _images(n), _poses(n), _rows9(n), **kw)


def _raises(root, pattern, exc=ValueError, **kw):
    with pytest.raises(exc, match=pattern):
        data.load_nerfstudio_split(root, "train", eval_mode="all", **kw)


# ------------------------------------------------------------------------------------------------ refusals and opt-ins
def test_with_the_opt_ins_off_every_refusal_of_today_is_raised_and_with_them_on_the_captures_load(tmp_path):
    name = "images/frame_00002.png"
    fisheye = _old_capture(tmp_path, "fisheye", frame_extra={2: {"camera_model": "OPENCV_FISHEYE", "p1": 0.0, "p2": 0.0}})
    _raises(fisheye, f"{name}.*OPENCV_FISHEYE")
    _raises(fisheye, f"{name}.*OPENCV_FISHEYE", masks=True, downscale_factor=1)  # the other opt-ins do not let it in
    fisheye_global = _old_capture(tmp_path, "fisheye_global", extra={"camera_model": "OPENCV_FISHEYE"})
    _raises(fisheye_global, "frame_00000.png.*OPENCV_FISHEYE")
    k4 = _old_capture(tmp_path, "k4", frame_extra={2: {"k4": 1e-3}})
    _raises(k4, f"{name}.*k4")
    from PIL import Image

    mask = _old_capture(tmp_path, "mask", frame_extra={2: {"mask_path": "masks/m.png"}})
    _raises(mask, f"{name}.*mask")
    _raises(mask, f"{name}.*mask", fisheye=True)
    # on: the same directories load
    sc = data.load_nerfstudio_split(fisheye, "train", eval_mode="all", **ON)
    assert sc.cameras.shape == (4, 12) and sc.cameras[:, 10].tolist() == [0.0, 0.0, 1.0, 0.0] and sc.masks is None
    _raises(fisheye_global, "frame_00000.png.*p1", **ON)  # the rows of this writer have tangential terms: a fisheye row must not
    _raises(k4, f"{name}.*k4.*perspective", **ON)  # a perspective row keeps k4 = 0
    _raises(mask, "m.png", exc=FileNotFoundError, **ON)
    os.makedirs(os.path.join(mask, "masks"))
    Image.fromarray(np.full((H + 1, W), 255, np.uint8)).save(os.path.join(mask, "masks", "m.png"))
    _raises(mask, f"{name}.*mask.*{W} x {H + 1}", **ON)
    live = np.zeros((H, W), np.uint8)
    live[3:9, 5:20] = 255
    Image.fromarray(live).save(os.path.join(mask, "masks", "m.png"))
    sc = data.load_nerfstudio_split(mask, "train", eval_mode="all", **ON)
    assert sc.masks.dtype == np.uint8 and sc.masks.shape == (4, H, W) and sc.cameras.shape == (4, 9)
    assert np.array_equal(sc.masks[2], (live != 0).astype(np.uint8)) and sc.masks[[0, 1, 3]].all()  # frames without a mask are all live
    # differing sizes and unknown models stay refused with everything on
    _raises(_old_capture(tmp_path, "equi", frame_extra={1: {"camera_model": "EQUIRECTANGULAR"}}), "frame_00001.png.*EQUIRECTANGULAR", **ON)


def test_the_twelve_column_table_and_the_nine_column_one(tmp_path):
    n = 4
    rows = [ref.fisheye_row(W, H), ref.perspective_row12(W, H), ref.fisheye_row(W, H, coeffs=(0, 0, 0, 0)), ref.perspective_row12(W, H, scale=1.1)]
    root = ref.write_lens_capture(str(tmp_path / "mixed"), _images(n), _poses(n), rows)
    sc = data.load_nerfstudio_split(root, "train", **RAW, **ON)
    assert data.LENS_CAMERA_COLUMNS == ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2", "k4", "model", "pad")
    assert sc.cameras.dtype == np.float32 and np.array_equal(sc.cameras, np.stack(rows).astype(np.float32))
    assert (sc.fx, sc.cx) == (float(sc.cameras[0, 0]), float(sc.cameras[0, 2]))
    with pytest.raises(ValueError, match="shared pinhole"):
        data.shared_pinhole(sc, "the point-cloud export")
    # no fisheye row among the kept frames: the table it always had, and the scene of a call without the arguments
    root = ref.write_lens_capture(str(tmp_path / "plain"), _images(n), _poses(n), [r[:9] for r in rows[1::2]] * 2)
    a, b = data.load_nerfstudio_split(root, "train", **RAW, **ON), data.load_nerfstudio_split(root, "train", **RAW)
    assert a.cameras.shape == (n, 9) and np.array_equal(a.cameras, b.cameras) and np.array_equal(a.images, b.images) and a.masks is None
    # a fisheye row with tangential terms is refused by name
    bad = ref.fisheye_row(W, H)
    bad[7] = 1e-3
    _raises(ref.write_lens_capture(str(tmp_path / "p1"), _images(2), _poses(2), [rows[1], bad]), "frame_00001.png.*p1", **ON)


def test_masks_follow_the_first_channel_in_every_file_mode(tmp_path):
    n = 4
    masks = {i: m for i, m in zip((0, 1, 3), ref.named_masks(3, H, W)["random30"])}
    root = ref.write_lens_capture(str(tmp_path / "cap"), _images(n), _poses(n), _rows9(n), masks=masks, mask_modes={0: "L", 1: "RGB", 3: "RGBA"})
    sc = data.load_nerfstudio_split(root, "train", **RAW, masks=True)
    assert sc.masks.shape == (n, H, W) and set(np.unique(sc.masks)) == {0, 1}
    for i in (0, 1, 3):
        assert np.array_equal(sc.masks[i], masks[i]), i
    assert sc.masks[2].all()
    assert data.load_nerfstudio_split(root, "train", **RAW, masks=True, pixels=False).masks is None  # cameras alone
    same = data.BlenderScene.from_arrays(sc.images, sc.c2w, focal=30.0, masks=sc.masks * 7)
    assert np.array_equal(same.masks, sc.masks)
    with pytest.raises(ValueError, match="masks must be"):
        data.BlenderScene.from_arrays(sc.images, sc.c2w, focal=30.0, masks=sc.masks[:, :-1])


def test_downscale_factor_reads_images_k_and_masks_k_with_the_intrinsics_over_k(tmp_path):
    n, K = 3, 2
    rows, poses = _rows9(n), _poses(n)
    full, half = _images(n, 5, 2 * H + 1, 2 * W + 1), _images(n, 6)  # 73 x 105 declared: 73 // 2 = 36, the truncation
    mk = {1: ref.named_masks(1, H, W)["rectangle"][0]}
    root = str(tmp_path / "cap")
    ref.write_lens_capture(root, half, poses, rows, masks=mk, image_dir="images_2", mask_dir="masks_2", declared_scale=K)
    meta = json.load(open(os.path.join(root, "transforms.json")))
    for fr in meta["frames"]:
        fr["w"], fr["h"] = 2 * W + 1, 2 * H + 1
    json.dump(meta, open(os.path.join(root, "transforms.json"), "w"))
    from PIL import Image

    os.makedirs(os.path.join(root, "images"))
    os.makedirs(os.path.join(root, "masks"))
    for i in range(n):
        Image.fromarray(full[i]).save(os.path.join(root, "images", f"frame_{i:05d}.png"))
    Image.fromarray(np.zeros((2 * H + 1, 2 * W + 1), np.uint8)).save(os.path.join(root, "masks", "frame_00001.png"))
    sc = data.load_nerfstudio_split(root, "train", **RAW, masks=True, downscale_factor=K)
    assert np.array_equal(sc.images[..., :3], half) and np.array_equal(sc.masks[1], mk[1]) and sc.masks[0].all()
    want = rows.copy()  # the JSON holds the rows' intrinsics times K; the loader divides them again
    assert np.array_equal(sc.cameras, (np.concatenate([want[:, :4] * K / K, want[:, 4:]], axis=1)).astype(np.float32))
    big = data.load_nerfstudio_split(root, "train", **RAW, masks=True)
    assert np.array_equal(big.images[..., :3], full) and np.array_equal(big.cameras[:, :4], (rows[:, :4] * K).astype(np.float32))
    assert not big.masks[1].any()
    # K = 1 is the call without the argument, array for array
    one = data.load_nerfstudio_split(root, "train", **RAW, masks=True, downscale_factor=1)
    for k in ("images", "c2w", "cameras", "masks", "dataparser_transform"):
        assert np.array_equal(getattr(one, k), getattr(big, k)), k
    assert (one.fx, one.fy, one.cx, one.cy, one.file_paths, one.dataparser_scale) == (big.fx, big.fy, big.cx, big.cy, big.file_paths, big.dataparser_scale)
    with pytest.raises(FileNotFoundError, match=r"images_4.*ns-process-data"):
        data.load_nerfstudio_split(root, "train", **RAW, masks=True, downscale_factor=4)
    with pytest.raises(ValueError, match="downscale_factor"):
        data.load_nerfstudio_split(root, "train", **RAW, downscale_factor=0)
    meta["frames"][2]["w"] = 2 * W + 2  # 106 // 2 = 53, not the file's 52
    json.dump(meta, open(os.path.join(root, "transforms.json"), "w"))
    _raises(root, "frame_00002.png.*106 x 73", downscale_factor=K, masks=True)


# ------------------------------------------------------------------------------------------------ the fisheye model
FISHEYE_TEST_ROWS = {
    "mild": lambda: ref.fisheye_row(W, H),
    "beyond_90": lambda: ref.fisheye_row(W, H, corner_theta_d=2.2),
    "on_axis": lambda: ref.fisheye_row(W, H, cx=20.5, cy=11.5),
    "equidistant": lambda: ref.fisheye_row(W, H, coeffs=(0.0, 0.0, 0.0, 0.0)),
}


def test_the_fisheye_reference_inverts_its_own_forward_model_and_the_loader_states_the_same_model():
    for name, make in FISHEYE_TEST_ROWS.items():
        row = make()
        theta = np.linspace(0.0, 2.4 if name == "beyond_90" else 1.5, 4001)
        td = ref.fisheye_forward(row, theta)
        assert np.all(np.diff(td) > 0.0), name
        back, res = ref.fisheye_inverse(row, td)
        assert np.abs(back - theta).max() <= 1e-12 and res.max() <= 1e-14, name
        assert np.abs(ref.newton_theta(row, td) - theta).max() <= 1e-12, name  # ten Newton steps get there too
        assert np.abs(data.fisheye_forward(row, theta) - td).max() <= 1e-15
        assert np.array_equal(np.clip(data.fisheye_solve(row, td), 0.0, math.pi), ref.newton_theta(row, td))
        assert data.fisheye_residual(row, H, W) <= 1e-12, name  # the loader's check accepts every test row
    # the geometry: theta_d = 0 looks down the axis, the beyond_90 corners look backwards
    row = FISHEYE_TEST_ROWS["on_axis"]()
    assert np.array_equal(ref.fisheye_camera_direction(row, 11 + 0.5, 20 + 0.5), [0.0, 0.0, -1.0])  # the centre of pixel (11, 20)
    row = FISHEYE_TEST_ROWS["beyond_90"]()
    assert ref.fisheye_camera_direction(row, 0.5, W - 0.5)[2] > 0.0 and ref.fisheye_camera_direction(row, H / 2, W / 2)[2] < 0.0
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    _, d, area = ref.rays(np.eye(4)[:3], row, yy, xx)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() <= 1e-15 and area.min() > 0.0


def test_the_load_time_check_rejects_a_fisheye_row_that_folds_inside_the_corners(tmp_path):
    # theta (1 + k1 theta^2) peaks at theta = 1 / sqrt(-3 k1): k1 = -0.3 -> theta = 1.054, theta_d = 0.703, inside the corner's 1.4
    fold = ref.fisheye_row(W, H, coeffs=(-0.3, 0.0, 0.0, 0.0))
    peak = 1.0 / math.sqrt(0.9)
    assert ref.fisheye_forward(fold, peak) < 1.4 and ref.fisheye_forward(fold, peak + 0.01) < ref.fisheye_forward(fold, peak)
    assert data.fisheye_residual(fold, H, W) == math.inf
    # a k2 that brings the curve back up to the corner's theta_d: f' = (1 - theta^2)(1 - 2 theta^2) is negative between 0.707 and 1,
    # so two angles share a radius whatever the corners' own solves find; the monotonicity scan refuses it
    fold2 = ref.fisheye_row(W, H, coeffs=(-1.0, 0.4, 0.0, 0.0), corner_theta_d=1.4)
    th = np.linspace(0.0, 1.6, 1601)
    assert np.any(np.diff(ref.fisheye_forward(fold2, th)) < 0.0) and ref.fisheye_forward(fold2, 1.6) > 1.4
    assert data.fisheye_residual(fold2, H, W) == math.inf
    root = ref.write_lens_capture(str(tmp_path / "fold"), _images(3), _poses(3), [ref.fisheye_row(W, H), ref.fisheye_row(W, H), fold])
    _raises(root, "frame_00002.png.*not invertible", **ON)
    # theta beyond pi: an fx so small that the corner's theta_d has no theta <= pi under the pure equidistant model
    far = ref.fisheye_row(W, H, coeffs=(0.0, 0.0, 0.0, 0.0), corner_theta_d=3.3)
    assert data.fisheye_residual(far, H, W) == math.inf


# ------------------------------------------------------------------------------------------------ the list rule
def test_a_level_pixel_is_live_only_when_every_pixel_under_it_is():
    masks = ref.named_masks(5, H, W)
    rect = masks["rectangle"]
    live = [ref.level_liveness(rect, l) for l in range(3)]
    # rows 5 .. 29 and columns 3 .. 42 are live: level 1 keeps rows 3 .. 14 (6 .. 29) and columns 2 .. 20, level 2 rows 2 .. 6, columns 1 .. 9
    assert live[0][0].sum() == 25 * 40 and live[1][0].sum() == 12 * 19 and live[2][0].sum() == 5 * 9
    assert live[1][0, 3:15, 2:21].all() and live[2][0, 2:7, 1:10].all()
    assert live[0][0].sum() > 4 * live[1][0].sum() > 16 * live[2][0].sum()  # the ragged border shrinks every coarser level
    for l in (1, 2):
        s = 1 << l
        for y, x in ((0, 0), (2, 1), (3, 2), (H // s - 1, W // s - 1)):
            assert live[l][0, y, x] == rect[0, y * s:(y + 1) * s, x * s:(x + 1) * s].all()
    one_dead = np.ones((1, 8, 8), np.uint8)
    one_dead[0, 5, 6] = 0
    assert ref.level_liveness(one_dead, 2)[0].tolist() == [[True, True], [True, False]]  # 15 of its 16 live: not enough
    lists = ref.live_lists(masks["dead_image"], 3)
    for l, lst in enumerate(lists):
        per = (H >> l) * (W >> l)
        assert lst.dtype == np.uint32 and len(lst) == 4 * per and not np.any((lst >= 2 * per) & (lst < 3 * per)) and np.all(np.diff(lst.astype(np.int64)) > 0)
    assert [len(x) for x in ref.live_lists(masks["last_pixel"], 3)] == [1, 0, 0]
    lvl, idx = ref.sample_through_lists(5, H, W, 3, None, 512, 7, 1, 3)
    from tests.pyramid_reference import sample_levels_and_indices

    old_lvl, old_idx = sample_levels_and_indices(5, H, W, 3, 512, 7, 1, 3)
    assert np.array_equal(lvl, old_lvl) and np.array_equal(idx, old_idx)  # without lists: the pyramid sampler's draw
    full = ref.live_lists(masks["all_live"], 3)
    assert np.array_equal(ref.sample_through_lists(5, H, W, 3, full, 512, 7, 1, 3)[1], old_idx)  # and with all-live lists too


# ------------------------------------------------------------------------------------------------ ABI, parser, checkpoint
def test_abi_declares_and_binds_the_new_calls():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rsn.h")).read()
    lib = _abi.load_library()
    for name in ("rsn_live_pixels_workspace_bytes", "rsn_build_live_pixels", "rsn_sample_capture_rays_live", "rsn_capture_rays_image2"):
        assert name + "(" in header and name in _abi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    cap, live = _abi._SIGNATURES["rsn_sample_capture_rays"][1], _abi._SIGNATURES["rsn_sample_capture_rays_live"][1]
    assert len(live) == len(cap) + 3 and live[:9] == cap[:9] and live[12:] == cap[9:]  # the stride and the two list pointers, after the table
    assert lib.rsn_abi_version() == 18
    # argument errors are host work: no launch, no device
    assert lib.rsn_live_pixels_workspace_bytes(5, 36, 52, 3) == 4 * (-(-9360 // 256) + -(-2340 // 256) + -(-585 // 256))
    assert lib.rsn_live_pixels_workspace_bytes(5, 36, 50, 3) == 0 and b"divisible" in lib.rsn_last_error()
    assert lib.rsn_build_live_pixels(5, 36, 52, 3, None, None, 0, None, None, 0, None) != 0 and b"NULL" in lib.rsn_last_error()
    assert lib.rsn_capture_rays_image2(8, 8, None, None, 10, None, None, None, None) != 0 and b"camera_stride" in lib.rsn_last_error()
    args = (1, 8, 8, 1, None, None, 0, None, None)
    tail = (0, 0, 0, None, None, None, None, None, None, None)
    assert lib.rsn_sample_capture_rays_live(*args, 12, None, None, 0, *tail) == 0  # no rays: nothing to do
    assert lib.rsn_sample_capture_rays_live(*args, 10, None, None, 0, *tail) != 0 and b"camera_stride" in lib.rsn_last_error()
    assert "#define RSN_LIVE_SCAN_CHUNK 65536" in header and "#define RSN_LIVE_TILE 256" in header


def test_parser_refuses_a_zero_downscale_factor_and_the_checkpoint_round_trips_the_setting(tmp_path, capsys):
    ap = trainer.build_parser()
    for bad in ("0", "-2", "1.5"):
        with pytest.raises(SystemExit):
            ap.parse_args(["train", "--data", "d", "--out", "o", "--downscale-factor", bad])
    assert "--downscale-factor" in capsys.readouterr().err
    args = ap.parse_args(["train", "--data", "d", "--out", "o", "--downscale-factor", "2"])
    kwargs, settings = trainer.capture_load_args(args)
    assert kwargs["downscale_factor"] == 2 and settings == {**trainer.CAPTURE_DATA_DEFAULTS, "downscale_factor": 2}
    # nothing given: the record a capture always had, no new key
    plain = ap.parse_args(["train", "--data", "d", "--out", "o"])
    kwargs, settings = trainer.capture_load_args(plain)
    assert settings == trainer.CAPTURE_DATA_DEFAULTS and kwargs == settings
    # the checkpoint's record decides for eval / render / a resumed run; a flag overrides it
    import torch

    state = checkpoint.make_run_state(0, 64, "f32", False, torch.device("cpu"),
                                      **{"data": {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS, "downscale_factor": 2,
                                                  "transform": np.eye(4)[:3].tolist(), "scale": 0.5}})
    path = str(tmp_path / "step-000000000.ckpt")
    torch.save({checkpoint.RUN_STATE_KEY: state, "step": 0}, path)
    rec = checkpoint.read_run_state(path)
    assert rec["data"]["downscale_factor"] == 2
    ev = ap.parse_args(["eval", "--data", "d", "--ckpt", path])
    kwargs, settings = trainer.capture_load_args(ev, rec)
    assert kwargs["downscale_factor"] == 2 and settings["downscale_factor"] == 2 and kwargs["applied"][1] == 0.5
    ev = ap.parse_args(["eval", "--data", "d", "--ckpt", path, "--downscale-factor", "1"])
    kwargs, settings = trainer.capture_load_args(ev, rec)
    assert "downscale_factor" not in kwargs and "downscale_factor" not in settings
    assert "--downscale-factor" in trainer.capture_flags_given(ev) and trainer.capture_flags_given(plain) == []
