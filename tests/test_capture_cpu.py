"""CPU checks of the nerfstudio-format (capture) input side: the float64 reference of tests/capture_reference.py against itself, the
loader's rules on scenes written to tmp_path, the pose normalisation, every rejected input, format detection, and the run-state
keys a capture adds to a checkpoint (and a Blender-format run does not)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, checkpoint, data, trainer
from tests import capture_reference as ref

H, W = 37, 53


def _poses(n, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([ref.look_at(rng.normal(size=3) * 2.0 + np.array([0.0, 0.0, 3.0])) for _ in range(n)])


def _images(n, seed=0, channels=3):
    return np.random.default_rng(seed).integers(0, 256, size=(n, H, W, channels), dtype=np.uint8)


def _rows(n, distorted=True):
    rows = np.stack([ref.camera_row(W, H, scale=1.0 + 0.01 * i) for i in range(n)])
    if not distorted:
        rows[:, 4:] = 0.0
    return rows


def _capture(tmp_path, n=6, **kw):
    rows = kw.pop("rows", _rows(n))
    poses = kw.pop("poses", _poses(n))
    return ref.write_capture(str(tmp_path / kw.pop("name", "cap")), kw.pop("images", _images(n)), poses, rows, **kw), rows, poses


# ------------------------------------------------------------------------------------------------ the reference and the loader's maths
def test_reference_undistort_inverts_distort_over_the_image():
    row = ref.camera_row(W, H)
    yy, xx = np.meshgrid(np.arange(-1, H + 2), np.arange(-1, W + 2), indexing="ij")  # the image and the neighbours' ring
    X, Y = ref.camera_point(row, yy, xx)  # asserts its own residual < 1e-15
    bx, by = ref.distort(row, X, Y)
    X2, Y2, res = ref.undistort(row, bx, by)
    assert max(np.abs(X2 - X).max(), np.abs(Y2 - Y).max()) <= 1e-12 and res.max() < 1e-15
    # the loader's statement of the model and of the kernel's ten-step solve agree with the reference's
    lx, ly = data.distort_points(row, X, Y)
    assert np.array_equal(lx, bx) and np.array_equal(ly, by)
    kx, ky = data.undistort_points(row, bx, by)
    assert max(np.abs(kx - X).max(), np.abs(ky - Y).max()) <= 1e-12
    assert data.undistort_residual(row, H, W) <= 1e-12


def test_abi_declares_and_binds_the_capture_calls():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "rsn.h")).read()
    lib = _abi.load_library()
    for name in ("rsn_sample_capture_rays", "rsn_capture_rays_image"):
        assert name + "(" in header and name in _abi.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    pyr, cap = _abi._SIGNATURES["rsn_sample_pyramid_rays"][1], _abi._SIGNATURES["rsn_sample_capture_rays"][1]
    assert cap == pyr[:8] + [_abi._fp] + pyr[12:]  # the pyramid sampler's list with the table in place of the four intrinsics
    assert lib.rsn_abi_version() == 18
    # argument errors are host work: no launch, no device
    assert lib.rsn_sample_capture_rays(1, 8, 8, 0, None, None, 0, None, None, 4, 0, 0, 0, None, None, None, None, None, None, None) != 0
    assert lib.rsn_sample_capture_rays(1, 8, 8, 1, None, None, 0, None, None, 0, 0, 0, 0, None, None, None, None, None, None, None) == 0
    assert lib.rsn_sample_capture_rays(1, 8, 8, 1, None, None, 0, None, None, 4, 0, 0, 0, None, None, None, None, None, None, None) != 0
    assert b"NULL" in lib.rsn_last_error()  # n_rays > 0 without buffers; the level pointer alone may be NULL at levels == 1
    assert lib.rsn_capture_rays_image(0, 8, None, None, None, None, None, None) != 0
    assert lib.rsn_capture_rays_image(8, 8, None, None, None, None, None, None) != 0


# ------------------------------------------------------------------------------------------------ loader
def test_global_and_per_frame_intrinsics_and_override(tmp_path):
    n = 6
    rows = _rows(n)
    rows[:] = rows[0]
    root_g, _, poses = _capture(tmp_path, n, rows=rows, per_frame=False, name="global")
    root_f, _, _ = _capture(tmp_path, n, rows=rows, per_frame=True, name="frames")
    g = data.load_nerfstudio_split(root_g, "train", eval_mode="all")
    f = data.load_nerfstudio_split(root_f, "train", eval_mode="all")
    assert g.cameras.dtype == np.float32 and g.cameras.shape == (n, 9)
    assert np.array_equal(g.cameras, np.tile(rows[0].astype(np.float32), (n, 1))) and np.array_equal(g.cameras, f.cameras)
    assert np.array_equal(g.c2w, f.c2w) and np.array_equal(g.images, f.images)
    assert (g.fx, g.fy, g.cx, g.cy) == tuple(float(v) for v in rows[0, :4].astype(np.float32))
    # a frame's value wins over the global one; coefficients that are absent are 0
    root_o, _, _ = _capture(tmp_path, n, rows=rows, per_frame=False, name="override",
                            frame_extra={2: {"fl_x": 77.0, "k1": 0.01}, 4: {"cx": 20.0}})
    meta = json.load(open(os.path.join(root_o, "transforms.json")))
    for k in ("k3", "p2"):
        del meta[k]
    json.dump(meta, open(os.path.join(root_o, "transforms.json"), "w"))
    o = data.load_nerfstudio_split(root_o, "train", eval_mode="all")
    want = np.tile(rows[0], (n, 1))
    want[:, 6] = 0.0
    want[:, 8] = 0.0
    want[2, 0], want[2, 4], want[4, 2] = 77.0, 0.01, 20.0
    assert np.array_equal(o.cameras, want.astype(np.float32))


def test_frames_are_sorted_by_name_and_png_and_jpeg_are_read(tmp_path):
    names = ["images/b.png", "images/a10.jpg", "images/a2.png", "images/c.png"]
    ims = _images(4)
    ims[1] = 128 + (np.arange(W)[None, :, None] // 8) * 4  # smooth: JPEG keeps it within a few levels
    root, rows, poses = _capture(tmp_path, 4, images=ims, names=names)
    sc = data.load_nerfstudio_split(root, "train", eval_mode="all", orientation="none", center="none", auto_scale=False)
    order = [1, 2, 0, 3]  # plain string sort: a10.jpg < a2.png < b.png < c.png
    assert sc.file_paths == [names[i] for i in order]
    assert np.array_equal(sc.cameras, rows[order].astype(np.float32))
    assert np.array_equal(sc.c2w, poses[order].astype(np.float32))
    assert sc.images.shape == (4, H, W, 4) and sc.images.dtype == np.uint8 and (sc.images[..., 3] == 255).all()
    assert np.array_equal(sc.images[1, ..., :3], ims[2]) and np.array_equal(sc.images[2, ..., :3], ims[0])  # PNG: exact
    assert np.abs(sc.images[0, ..., :3].astype(int) - ims[1].astype(int)).max() <= 6  # JPEG quality 95 of a smooth image
    # RGBA PNGs keep their alpha; headers-only loading runs the same checks and decodes nothing
    root4, _, _ = _capture(tmp_path, 3, images=_images(3, channels=4), name="rgba")
    assert np.array_equal(data.load_nerfstudio_split(root4, "train", eval_mode="all").images, _images(3, channels=4))
    lazy = data.load_nerfstudio_split(root, "train", eval_mode="all", pixels=False)
    assert lazy.images.shape == (4, H, W, 4) and lazy.images.strides == (0, 0, 0, 0) and np.array_equal(lazy.cameras, sc.cameras)


@pytest.mark.parametrize("n", [10, 23])
def test_split_indices_follow_the_written_rule(tmp_path, n):
    root, rows, _ = _capture(tmp_path, n)
    i_train, i_eval = ref.split_indices(n, 0.9)
    assert len(i_train) == math.ceil(0.9 * n) and sorted(set(i_train) | set(i_eval)) == list(range(n)) and not set(i_train) & set(i_eval)
    if n == 10:
        assert list(i_train) == [0, 1, 2, 3, 4, 5, 6, 7, 9] and list(i_eval) == [8]
    assert np.array_equal(data.capture_split_indices(n, "train"), i_train)
    names = [f"images/frame_{i:05d}.png" for i in range(n)]
    tr = data.load_nerfstudio_split(root, "train")
    assert tr.file_paths == [names[i] for i in i_train] and np.array_equal(tr.cameras, rows[i_train].astype(np.float32))
    for split in ("val", "test"):
        assert data.load_nerfstudio_split(root, split).file_paths == [names[i] for i in i_eval]
    half_train, half_eval = ref.split_indices(n, 0.5)
    assert data.load_nerfstudio_split(root, "test", train_split_fraction=0.5).file_paths == [names[i] for i in half_eval]
    for split in ("train", "test"):  # eval_mode all: every split gets every frame
        assert data.load_nerfstudio_split(root, split, eval_mode="all").file_paths == names
    # the normalisation is computed over ALL frames before the split: a frame has one pose whatever split it is read in
    every = data.load_nerfstudio_split(root, "train", eval_mode="all")
    assert np.array_equal(tr.c2w, every.c2w[i_train]) and np.array_equal(data.load_nerfstudio_split(root, "val").c2w, every.c2w[i_eval])


def test_pose_normalisation_properties(tmp_path):
    n = 9
    root, _, poses = _capture(tmp_path, n)
    sc = data.load_nerfstudio_split(root, "train", eval_mode="all", scale_factor=0.7)
    P = sc.c2w.astype(np.float64)
    up = P[:, :, 1].mean(0)
    assert np.abs(up / np.linalg.norm(up) - [0, 0, 1]).max() <= 1e-6
    assert np.abs(P[:, :, 3].mean(0)).max() <= 1e-6
    assert abs(np.abs(P[:, :, 3]).max() - 0.7) <= 1e-6  # max |t|: the largest absolute translation component, nerfstudio's rule
    # against the restatement, and the recorded transform and scale reproduce the poses
    want, transform = ref.orient_and_center(poses)
    scale = 0.7 / np.abs(want[:, :, 3]).max()
    want[:, :, 3] *= scale
    assert np.abs(P - want).max() <= 1e-6
    assert np.abs(sc.dataparser_transform - transform).max() <= 1e-12 and abs(sc.dataparser_scale - scale) <= 1e-12 * scale
    again = data.load_nerfstudio_split(root, "train", eval_mode="all", applied=(sc.dataparser_transform, sc.dataparser_scale),
                                       orientation="none", center="none", auto_scale=False)
    assert np.array_equal(again.c2w, sc.c2w)
    for i in range(n):  # rotations stay rotations
        assert np.abs(P[i, :, :3].T @ P[i, :, :3] - np.eye(3)).max() <= 1e-6
    # the "none" variants leave the poses as they were (auto_scale off: times scale_factor alone)
    raw = data.load_nerfstudio_split(root, "train", eval_mode="all", orientation="none", center="none", auto_scale=False)
    assert np.array_equal(raw.c2w, poses.astype(np.float32)) and raw.dataparser_scale == 1.0
    assert np.array_equal(raw.dataparser_transform, np.eye(4)[:3])
    only_center = data.load_nerfstudio_split(root, "train", eval_mode="all", orientation="none", auto_scale=False).c2w
    assert np.array_equal(only_center[:, :, :3], poses.astype(np.float32)[:, :, :3]) and np.abs(only_center[:, :, 3].mean(0)).max() <= 1e-6
    only_up = data.load_nerfstudio_split(root, "train", eval_mode="all", center="none", auto_scale=False).c2w.astype(np.float64)
    assert np.abs(np.linalg.norm(only_up[:, :, 3], axis=1) - np.linalg.norm(poses[:, :, 3], axis=1)).max() <= 1e-5


def test_antiparallel_up_is_a_turn_of_pi_about_x(tmp_path):
    assert np.array_equal(data.rotation_onto_z([0.0, 0.0, -1.0]), np.diag([1.0, -1.0, -1.0]))
    assert np.array_equal(data.rotation_onto_z([0.0, 0.0, 1.0]), np.eye(3))
    down = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])  # a rotation whose up axis, column 1, is -z
    poses = np.stack([np.concatenate([down, [[float(i)], [0.0], [1.0]]], axis=1) for i in range(4)])
    root, _, _ = _capture(tmp_path, 4, poses=poses)
    sc = data.load_nerfstudio_split(root, "train", eval_mode="all", center="none", auto_scale=False)
    assert np.array_equal(sc.c2w[:, :, 1], np.tile(np.float32([0, 0, 1]), (4, 1)))
    assert np.array_equal(sc.c2w[:, :, 3], np.float32([[i, 0, -1] for i in range(4)]))
    rng = np.random.default_rng(3)
    for _ in range(20):  # Rodrigues: a proper rotation that takes up onto +z
        up = rng.normal(size=3)
        up /= np.linalg.norm(up)
        R = data.rotation_onto_z(up)
        assert np.abs(R @ up - [0, 0, 1]).max() <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0


# ------------------------------------------------------------------------------------------------ rejected inputs
def _raises(root, match, exc=ValueError, **kw):
    with pytest.raises(exc, match=match):
        data.load_nerfstudio_split(root, "train", eval_mode="all", **kw)


def test_every_rejected_input_names_its_frame(tmp_path):
    name = "images/frame_00002.png"
    root, _, _ = _capture(tmp_path, 4, name="fisheye", frame_extra={2: {"camera_model": "OPENCV_FISHEYE"}})
    _raises(root, f"{name}.*OPENCV_FISHEYE")
    root, _, _ = _capture(tmp_path, 4, name="fisheye_global", extra={"camera_model": "OPENCV_FISHEYE"})
    _raises(root, "frame_00000.png.*OPENCV_FISHEYE")
    root, _, _ = _capture(tmp_path, 4, name="k4", frame_extra={2: {"k4": 1e-3}})
    _raises(root, f"{name}.*k4")
    root, _, _ = _capture(tmp_path, 4, name="k4zero", extra={"k4": 0.0, "camera_model": "PINHOLE"})
    data.load_nerfstudio_split(root, "train", eval_mode="all")  # a zero k4 and PINHOLE are fine
    root, _, _ = _capture(tmp_path, 4, name="mask", frame_extra={2: {"mask_path": "masks/m.png"}})
    _raises(root, f"{name}.*mask")
    root, _, _ = _capture(tmp_path, 4, name="wh", frame_extra={2: {"w": W + 1}})
    _raises(root, f"{name}.*{W + 1} x {H}")
    root, _, _ = _capture(tmp_path, 4, name="size")
    from PIL import Image

    Image.fromarray(np.zeros((H, W - 3, 3), np.uint8)).save(os.path.join(root, name))
    meta = json.load(open(os.path.join(root, "transforms.json")))
    for fr in meta["frames"]:
        del fr["w"], fr["h"]
    json.dump(meta, open(os.path.join(root, "transforms.json"), "w"))
    _raises(root, f"{name}.*differing sizes")
    root, _, _ = _capture(tmp_path, 4, name="missing")
    os.remove(os.path.join(root, name))
    _raises(root, "frame_00002.png", exc=FileNotFoundError)
    # a coefficient set whose solve does not converge at the image's border: k1 = -1.2 folds the image inside the corners
    rows = _rows(4)
    rows[2, 4:] = (-1.2, 0.0, 0.0, 0.0, 0.0)
    assert not ref.undistort(rows[2], *[np.array([v]) for v in ((0.5 - rows[2, 2]) / rows[2, 0], (0.5 - rows[2, 3]) / rows[2, 1])],
                             iterations=10)[2].max() <= 1e-9
    root, _, _ = _capture(tmp_path, 4, name="fold", rows=rows)
    _raises(root, f"{name}.*not invertible")
    with pytest.raises(ValueError, match="train_split_fraction"):
        data.load_nerfstudio_split(root, "train", train_split_fraction=0.0)


def test_format_detection(tmp_path):
    cap, _, _ = _capture(tmp_path, 3)
    assert data.detect_data_format(cap) == "nerfstudio" and data.detect_data_format(cap, "blender") == "blender"
    blender = tmp_path / "blender"
    blender.mkdir()
    (blender / "transforms_train.json").write_text("{}")
    assert data.detect_data_format(str(blender)) == "blender" and data.detect_data_format(str(blender), "nerfstudio") == "nerfstudio"
    (blender / "transforms.json").write_text("{}")
    assert data.detect_data_format(str(blender)) == "nerfstudio"
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="transforms.json"):
        data.detect_data_format(str(empty))
    with pytest.raises(ValueError):
        data.detect_data_format(cap, "colmap")
    ap = trainer.build_parser()
    a = ap.parse_args(["train", "--data", cap, "--out", "o"])
    assert a.data_format == "auto" and a.scale_factor == 1.0 and all(
        getattr(a, k) is None for k in ("orientation", "center_poses", "no_auto_scale", "train_split_fraction", "eval_mode", "near", "far",
                                        "primary_spacing", "primary_tan"))
    a = ap.parse_args(["train", "--data", cap, "--out", "o", "--orientation", "none", "--center", "none", "--no-auto-scale",
                       "--train-split-fraction", "0.5", "--eval-mode", "all", "--near", "0.5", "--far", "1.5", "--primary-spacing",
                       "reciprocal", "--primary-tan", "2", "--data-format", "nerfstudio"])
    kwargs, settings = trainer.capture_load_args(a)
    assert settings == {"orientation": "none", "center": "none", "auto_scale": False, "scale_factor": 1.0, "train_split_fraction": 0.5,
                        "eval_mode": "all"} and kwargs == settings
    with pytest.raises(SystemExit):  # the capture's flags on a Blender-format scene are an error, not ignored
        trainer.load_scene(ap, ap.parse_args(["train", "--data", str(tmp_path / "nowhere"), "--out", "o", "--data-format", "blender",
                                              "--orientation", "none"]), "train")
    with pytest.raises(ValueError, match="one shared pinhole"):
        data.shared_pinhole(data.load_nerfstudio_split(cap, "train", eval_mode="all"), "export-pointcloud")
    flat, _, _ = _capture(tmp_path, 3, name="flat", rows=np.tile(_rows(1, distorted=False), (3, 1)))
    sc = data.load_nerfstudio_split(flat, "train", eval_mode="all")
    assert data.shared_pinhole(sc, "export-pointcloud") == (sc.fx, sc.fy, sc.cx, sc.cy)


# ------------------------------------------------------------------------------------------------ checkpoint keys
def _small_cfg():
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=8, num_importance_samples=8, num_reflect_coarse_samples=4,
                                              num_reflect_importance_samples=4, base_mlp_num_layers=2, base_mlp_layer_width=16)


NEW_KEYS = ("near", "far", "primary_spacing", "primary_tan", "data")


def test_run_state_round_trip_of_the_new_keys_and_none_for_a_blender_run(tmp_path):
    model = trainer.make_model(_small_cfg(), seed=0)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    plain = checkpoint.make_run_state(0, 1024, "f32", False, "cpu")
    assert not set(NEW_KEYS) & set(plain)
    assert checkpoint.make_run_state(0, 1024, "f32", False, "cpu", **dict.fromkeys(NEW_KEYS)) .keys() == plain.keys()
    record = {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS, "transform": np.eye(4)[:3].tolist(), "scale": 0.25}
    rays = {"near": 0.5, "far": 1.5, "primary_spacing": "reciprocal", "primary_tan": 2.0}
    state = checkpoint.make_run_state(0, 1024, "f32", False, "cpu", **{**rays, "data": record})
    path = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "run"), 7), model, opt, 7, state)
    back = checkpoint.read_run_state(str(tmp_path / "run"))
    assert {k: back[k] for k in rays} == rays and back["data"] == record
    # every opener casts its rays the way the run did
    loaded, _ = checkpoint._load_pipeline(path, _small_cfg())
    assert loaded.config.collider_params == {"near_plane": 0.5, "far_plane": 1.5}
    assert (loaded.collider.near_plane, loaded.collider.far_plane) == (0.5, 1.5)
    spec = loaded.sampler_uniform.spec
    assert (spec.spacing, spec.tan, spec.num_samples) == (_abi.RSN_SPACING_RECIPROCAL, 2.0, 8)
    over, _ = checkpoint._load_pipeline(path, _small_cfg(), rays={"primary_spacing": "uniform", "far": 3.0, "near": None})
    assert over.sampler_uniform.spec.spacing == _abi.RSN_SPACING_UNIFORM and over.config.collider_params == {"near_plane": 0.5, "far_plane": 3.0}
    # a checkpoint without the keys: the config's own planes and the uniform sampler, as always
    old = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "old"), 7), model, opt, 7, plain)
    loaded, _ = checkpoint._load_pipeline(old, _small_cfg())
    assert loaded.config.collider_params == {"near_plane": 2.0, "far_plane": 6.0} and loaded.sampler_uniform.spec.spacing == _abi.RSN_SPACING_UNIFORM
    cfg = _small_cfg()
    assert checkpoint.config_with_planes(cfg) is cfg and checkpoint.config_with_planes(cfg, 0.5).collider_params["far_plane"] == 6.0
    assert cfg.collider_params == {"near_plane": 2.0, "far_plane": 6.0}
    with pytest.raises(ValueError):
        checkpoint.config_with_planes(cfg, 7.0)
    with pytest.raises(ValueError):
        checkpoint.set_primary_sampler(model, "log")
    # the flags of a command line: given > the checkpoint's record > the default; the recorded frame is applied as it is
    ap = trainer.build_parser()
    a = ap.parse_args(["eval", "--data", "d", "--ckpt", "c"])
    rec = {"data": {**record, "orientation": "none", "train_split_fraction": 0.5}}
    kwargs, settings = trainer.capture_load_args(a, rec)
    assert settings["orientation"] == "none" and settings["train_split_fraction"] == 0.5 and kwargs["applied"] == (record["transform"], 0.25)
    a = ap.parse_args(["eval", "--data", "d", "--ckpt", "c", "--center-poses", "none", "--eval-mode", "all"])
    kwargs, settings = trainer.capture_load_args(a, rec)
    assert "applied" not in kwargs and settings["center"] == "none" and settings["eval_mode"] == "all" and settings["orientation"] == "none"
    a = ap.parse_args(["eval", "--data", "d", "--ckpt", "c", "--scale-factor", "1.0"])
    assert "applied" not in trainer.capture_load_args(a, rec)[0]  # typed, even at the default's value: given
    assert trainer.capture_load_args(ap.parse_args(["eval", "--data", "d", "--ckpt", "c"]), None)[1] == trainer.CAPTURE_DATA_DEFAULTS


def test_render_and_export_cameras_of_a_capture_come_from_the_file_and_the_checkpoint(tmp_path):
    n = 6
    root, rows, poses = _capture(tmp_path, n)
    trained = data.load_nerfstudio_split(root, "train", eval_mode="all", scale_factor=0.5)
    record = {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS, "scale_factor": 0.5, "eval_mode": "all",
              "transform": trained.dataparser_transform.tolist(), "scale": trained.dataparser_scale}
    model = trainer.make_model(_small_cfg(), seed=0)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    run = str(tmp_path / "run")
    trainer.save_checkpoint(trainer.checkpoint_path(run, 3), model, opt, 3,
                            checkpoint.make_run_state(0, 1024, "f32", False, "cpu", **{"data": record}))
    ap = trainer.build_parser()
    cams = trainer.resolve_render_args(ap, ap.parse_args(["render", "--ckpt", run, "--out", "o", "--data", root]))
    # the file's frames (every one: the run's eval_mode) in the run's frame, through their own cameras
    assert np.array_equal(cams["c2w"], trained.c2w) and np.array_equal(cams["camera_table"], rows.astype(np.float32))
    assert (cams["width"], cams["height"]) == (W, H)
    orbit = trainer.resolve_render_args(ap, ap.parse_args(["render", "--ckpt", run, "--out", "o", "--data", root, "--path", "orbit", "--frames", "3"]))
    assert "camera_table" not in orbit and orbit["c2w"].shape == (3, 3, 4)
    assert tuple(orbit[k] for k in ("fx", "fy", "cx", "cy")) == tuple(float(v) for v in rows[0, :4].astype(np.float32))  # the first camera's pinhole part
    with pytest.raises(SystemExit):  # the frames' own cameras take no --fov-x
        trainer.resolve_render_args(ap, ap.parse_args(["render", "--ckpt", run, "--out", "o", "--data", root, "--fov-x", "40"]))
    with pytest.raises(SystemExit):  # one shared pinhole: a distorted capture is refused by the TSDF route
        trainer.resolve_export_cameras(ap, ap.parse_args(["export-mesh", "--method", "tsdf", "--ckpt", run, "--out", "m.ply", "--data", root]))
    flat, flat_rows, _ = _capture(tmp_path, n, name="flat", rows=np.tile(_rows(1, distorted=False), (n, 1)))
    ex = trainer.resolve_export_cameras(ap, ap.parse_args(["export-mesh", "--method", "tsdf", "--ckpt", run, "--out", "m.ply", "--data", flat,
                                                           "--max-views", "3", "--downscale", "2"]))
    assert ex["c2w"].shape == (3, 3, 4) and (ex["width"], ex["height"]) == (W // 2, H // 2)
    assert ex["fx"] == pytest.approx(float(np.float32(flat_rows[0, 0])) * (W // 2) / W)
