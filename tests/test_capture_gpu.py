"""GPU checks of the capture data path (include/rsn.h, "captures"): rsn_sample_capture_rays / rsn_capture_rays_image byte for byte
against the existing calls where a camera has no distortion, against the Philox restatement, against the float64 reference of
tests/capture_reference.py where it has, a host-sync-free data manager, and train -> checkpoint -> eval -> render -> resume end to
end on an analytically rendered capture with distorted per-frame cameras."""
import math
import os

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, checkpoint, data, render, trainer
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from tests import capture_reference as ref
from tests.data_reference import sample_indices
from tests.pyramid_reference import sample_levels_and_indices

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RAY_COUNTS = (1, 63, 1025)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _scene(N=5, H=37, W=53, rows=None, seed=0):
    """Random RGBA images and poses; rows: None (the shared pinhole of row 0, no table) or the camera table."""
    rng = np.random.default_rng(seed)
    ims = rng.integers(0, 256, size=(N, H, W, 4), dtype=np.uint8)
    poses = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        poses[i, :, :3] = _rot(*rng.uniform(-math.pi, math.pi, 3))
        poses[i, :, 3] = rng.normal(size=3) * 3.0
    k = ref.camera_row(W, H).astype(np.float32)
    return BlenderScene(images=ims, c2w=poses, fx=float(k[0]), fy=float(k[1]), cx=float(k[2]), cy=float(k[3]),
                        cameras=None if rows is None else np.ascontiguousarray(rows, dtype=np.float32))


def _mixed_rows(N, H, W):
    """Distorted rows with their own intrinsics at the even images, all-zero coefficients at the odd ones: one wave takes both paths."""
    rows = np.stack([ref.camera_row(W, H, scale=1.0 + 0.02 * i) for i in range(N)])
    rows[1::2, 4:] = 0.0
    return rows.astype(np.float32)


def _host(rb, b):
    torch.cuda.synchronize()
    out = {"origins": rb.origins, "directions": rb.directions, "pixel_area": rb.pixel_area, "image": b["image"], "indices": b["indices"]}
    if "levels" in b:
        out["levels"] = b["levels"]
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bytes(a, b, keys=None):
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 1. bit identity, zero coefficients
@pytest.mark.parametrize("N", [1, 5])
def test_zero_coefficient_table_has_the_existing_samplers_bytes(N):
    for levels, (H, W) in ((1, (37, 53)), (3, (40, 56))):
        plain = _scene(N, H, W)
        row = np.float32([plain.fx, plain.fy, plain.cx, plain.cy, 0, 0, 0, 0, 0])
        table = _scene(N, H, W, rows=np.tile(row, (N, 1)))
        for R in RAY_COUNTS:
            old = RayDataManager(plain, DEV, num_rays_per_batch=R, seed=77, rank=3, levels=levels)
            new = RayDataManager(table, DEV, num_rays_per_batch=R, seed=77, rank=3, levels=levels)
            assert old.cameras is None and new.cameras.shape == (levels, N, 9)
            for step in (0, 11):
                a, b = _host(*old.next_train(step)), _host(*new.next_train(step))
                assert ("levels" in a) == (levels > 1) and b["indices"].shape == (R, 3)
                _same_bytes(a, b)  # levels == 1: rsn_sample_camera_rays; levels == 3: rsn_sample_pyramid_rays
        for i in range(N):
            for level in range(levels):
                o, n = old.camera_ray_bundle(i, level), new.camera_ray_bundle(i, level)
                for k in ("origins", "directions", "pixel_area"):
                    assert torch.equal(getattr(o, k), getattr(n, k)), (i, level, k)


def test_per_image_pinholes_have_the_image_kernels_bytes():
    N, H, W = 5, 40, 56
    rows = _mixed_rows(N, H, W)
    rows[:, 4:] = 0.0  # per-image intrinsics, no distortion
    dm = RayDataManager(_scene(N, H, W, rows=rows), DEV, levels=2)
    for i in range(N):
        for level in range(2):
            fx, fy, cx, cy = (float(v) / (1 << level) for v in rows[i, :4])
            want = render.camera_rays(dm.c2w[i], H >> level, W >> level, fx, fy, cx, cy, DEV)  # rsn_camera_rays_image with four floats
            got = dm.camera_ray_bundle(i, level)
            for k in ("origins", "directions", "pixel_area"):
                assert torch.equal(getattr(want, k), getattr(got, k)), (i, level, k)


# ------------------------------------------------------------------------------------------------ 2. indices; sampler == image kernel
@pytest.mark.parametrize("N", [1, 5])
def test_indices_match_philox_and_sampled_rays_match_the_image_kernel_bitwise(N):
    for levels, (H, W) in ((1, (37, 53)), (3, (40, 56))):
        sc = _scene(N, H, W, rows=_mixed_rows(N, H, W))
        views = None
        for R in RAY_COUNTS:
            dm = RayDataManager(sc, DEV, num_rays_per_batch=R, seed=1234, rank=2, levels=levels)
            got = _host(*dm.next_train(17))
            if levels == 1:
                lvl, idx = np.zeros(R, np.int64), sample_indices(N, H, W, R, seed=1234, rank=2, step=17)
            else:
                lvl, idx = sample_levels_and_indices(N, H, W, levels, R, seed=1234, rank=2, step=17)
                assert np.array_equal(got["levels"], lvl)
            assert got["indices"].dtype == np.int32 and np.array_equal(got["indices"], idx)
            if views is None:
                views = {(i, l): dm.camera_ray_bundle(i, l) for i in range(N) for l in range(levels)}
                views = {k: tuple(getattr(v, n).cpu().numpy() for n in ("origins", "directions", "pixel_area")) for k, v in views.items()}
            for r in range(R):
                o, d, pa = views[(int(idx[r, 0]), int(lvl[r]))]
                y, x = int(idx[r, 1]), int(idx[r, 2])
                assert o[y, x].tobytes() == got["origins"][r].tobytes() and d[y, x].tobytes() == got["directions"][r].tobytes()
                assert pa[y, x].tobytes() == got["pixel_area"][r].tobytes()


# ------------------------------------------------------------------------------------------------ 3. distorted rays against float64
def measure_against_float64(N=5):
    """Every pixel of every camera at levels 0 and 1 (37 x 53: level 0 only, it has no level 1) -> the worst, over cameras and levels,
    of kernel error / (4 x the float32 restatement's error) for directions (largest absolute component error), pixel_area (relative
    error) and the landing point of the direction pushed forward through the float64 model (pixels); each camera and level has its
    own bound, from the restatement's error on its inputs.  Also the errors themselves.  tools/capture_report.py records it."""
    worst = {"direction": 0.0, "pixel_area": 0.0, "landing_px": 0.0}
    errors = {"direction": 0.0, "pixel_area_rel": 0.0, "landing_px": 0.0, "restatement_direction": 0.0, "restatement_pixel_area_rel": 0.0,
              "restatement_landing_px": 0.0}
    checked = 0
    for levels, (H, W) in ((1, (37, 53)), (2, (40, 56))):
        rows = _mixed_rows(N, H, W)
        sc = _scene(N, H, W, rows=rows)
        dm = RayDataManager(sc, DEV, levels=levels)
        tables = dm.cameras.cpu().numpy()
        for level in range(levels):
            h, w = H >> level, W >> level
            yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            for i in range(N):
                row32 = tables[level, i]
                assert np.array_equal(row32[:4], rows[i, :4] / np.float32(1 << level)) and np.array_equal(row32[4:], rows[i, 4:])
                row, pose = row32.astype(np.float64), sc.c2w[i].astype(np.float64)  # the reference works on the device's inputs
                o, d, area = ref.rays(pose, row, yy, xx)  # asserts the float64 solve's convergence at every pixel
                rd, ra = ref.rays_f32(sc.c2w[i], row32, yy, xx)
                rb = dm.camera_ray_bundle(i, level)
                go, gd, ga = (t.cpu().numpy() for t in (rb.origins, rb.directions, rb.pixel_area[..., 0]))
                assert np.array_equal(go, np.broadcast_to(sc.c2w[i][:, 3], (h, w, 3)))  # origins are exact

                def landing(dirs):
                    u, v = ref.project(pose, row, dirs)
                    return max(np.abs(u - (xx + 0.5)).max(), np.abs(v - (yy + 0.5)).max())

                pairs = {"direction": (np.abs(gd - d).max(), np.abs(rd - d).max()),
                         "pixel_area": ((np.abs(ga - area) / area).max(), (np.abs(ra - area) / area).max()),
                         "landing_px": (landing(gd), landing(rd))}
                for k, (got, restated) in pairs.items():
                    assert restated > 0.0
                    worst[k] = max(worst[k], got / (4.0 * restated))
                    name = k + "_rel" if k == "pixel_area" else k
                    errors[name] = max(errors[name], got)
                    errors["restatement_" + name] = max(errors["restatement_" + name], restated)
                checked += h * w
    return worst, errors, checked


def test_distorted_rays_match_float64_within_four_times_the_float32_restatements_error():
    worst, errors, checked = measure_against_float64()
    print(f"capture rays vs float64 over {checked} pixels: share of the bound (4 x the float32 restatement's error) "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + "; errors " + ", ".join(f"{k} {v:.3e}" for k, v in errors.items()))
    for k, share in worst.items():
        assert share <= 1.0, (k, share)


# ------------------------------------------------------------------------------------------------ 4. data manager
def _write_capture(tmp_path, N=5, H=40, W=56):
    sc = _scene(N, H, W, rows=_mixed_rows(N, H, W))
    root = ref.write_capture(str(tmp_path / "capture"), sc.images, sc.c2w, sc.cameras.astype(np.float64))
    return root, sc


def test_data_manager_on_a_written_capture_issues_no_host_sync(tmp_path):
    root, sc = _write_capture(tmp_path)
    loaded = data.load_nerfstudio_split(root, "train", eval_mode="all", orientation="none", center="none", auto_scale=False)
    assert np.array_equal(loaded.cameras, sc.cameras) and np.array_equal(loaded.c2w, sc.c2w) and np.array_equal(loaded.images, sc.images)
    for levels in (1, 2):
        dm = RayDataManager(loaded, DEV, num_rays_per_batch=1025, seed=5, levels=levels)
        want = _host(*RayDataManager(sc, DEV, num_rays_per_batch=1025, seed=5, levels=levels).next_train(3))
        dm.next_train(0), dm.camera_ray_bundle(0, levels - 1)  # warm-up: allocator growth
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            rb, b = dm.next_train(3)
            views = [dm.camera_ray_bundle(i, level) for i in (0, 4) for level in range(levels)]
        finally:
            torch.cuda.set_sync_debug_mode(0)
        _same_bytes(want, _host(rb, b))
        assert all(v.origins.shape == (40 >> l, 56 >> l, 3) for v, l in zip(views, list(range(levels)) * 2))
        assert bool(torch.isfinite(rb.directions).all()) and all(bool(torch.isfinite(v.pixel_area).all()) for v in views)


def test_without_a_table_the_data_manager_makes_the_old_calls():
    """Byte equality of a batch with the recipe the data manager had before captures: rsn_sample_camera_rays into one fp32
    allocation of four views and an int32 [R,3]; rsn_sample_pyramid_rays with the levels behind the indices."""
    lib = _abi.load_library()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for levels, (H, W) in ((1, (37, 53)), (3, (40, 56))):
        s = _scene(5, H, W)
        dm = RayDataManager(s, DEV, num_rays_per_batch=1025, seed=9, rank=1, levels=levels)
        rb, b = dm.next_train(4)
        got = _host(rb, b)
        R = 1025
        flat = torch.empty(R * 10, device=DEV, dtype=torch.float32)
        o, d, pa, rgb = flat[0:3 * R].view(R, 3), flat[3 * R:6 * R].view(R, 3), flat[6 * R:7 * R].view(R, 1), flat[7 * R:10 * R].view(R, 3)
        if levels == 1:
            idx = torch.empty(R, 3, device=DEV, dtype=torch.int32)
            _abi.check(lib.rsn_sample_camera_rays(s.num_images, H, W, _abi.ptr(dm.images), _abi.ptr(dm.c2w), s.fx, s.fy, s.cx, s.cy, R, 9, 1, 4,
                                                  _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa), _abi.ptr(rgb), _abi.ptr(idx), stream))
            assert set(b) == {"image", "indices"} and b["indices"].shape == (R, 3) and b["indices"].is_contiguous()
            want = {"origins": o, "directions": d, "pixel_area": pa, "image": rgb, "indices": idx}
        else:
            both = torch.empty(R * 4, device=DEV, dtype=torch.int32)
            idx, lvl = both[:3 * R].view(R, 3), both[3 * R:]
            _abi.check(lib.rsn_sample_pyramid_rays(s.num_images, H, W, levels, _abi.ptr(dm.images), _abi.ptr(dm.pyramid), dm.pyramid.shape[0],
                                                   _abi.ptr(dm.c2w), s.fx, s.fy, s.cx, s.cy, R, 9, 1, 4, _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa),
                                                   _abi.ptr(rgb), _abi.ptr(idx), _abi.ptr(lvl), stream))
            want = {"origins": o, "directions": d, "pixel_area": pa, "image": rgb, "indices": idx, "levels": lvl}
        torch.cuda.synchronize()
        _same_bytes({k: v.cpu().numpy() for k, v in want.items()}, got)
        assert b["image"].data_ptr() == rb.origins.data_ptr() + 7 * R * 4  # one allocation, four views, as before
        view = dm.camera_ray_bundle(2)
        old = render.camera_rays(dm.c2w[2], H, W, s.fx, s.fy, s.cx, s.cy, DEV)
        assert torch.equal(view.directions, old.directions) and torch.equal(view.pixel_area, old.pixel_area)


# ------------------------------------------------------------------------------------------------ 5. end to end
E2E_STEPS = 400
E2E_FRAMES = 26  # the 0.9 fraction split trains on ceil(23.4) = 24 of them and holds 2 out
# The existing Blender-format path on the parent commit, for this sphere at this scale -- the pinhole scene of tests/test_data_gpu.py
# with the translations times 0.25 (scale_factor 0.25) and the collider at 0.5 .. 1.5, 400 steps of the 4 x 64 config, four test views
# -- gains E2E_BLENDER_GAIN_DB of test-view PSNR on an MI355X (profiles/capture_rays.json).  The bound is half of that gain.
# Measured twice (the default mode's weight-gradient atomics make two runs differ): 6.23 -> 6.97 dB (+0.737) and 6.23 -> 6.98 dB
# (+0.750); the recorded run is the second.  This test's own, deterministic run: 5.71 -> 6.24 dB, a gain of 0.53 against the bound of 0.37.
E2E_BLENDER_GAIN_DB = 0.7497
E2E_MIN_GAIN_DB = 0.5 * E2E_BLENDER_GAIN_DB


def _cfg():
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                              num_reflect_importance_samples=16, base_mlp_num_layers=4, base_mlp_layer_width=64)


@pytest.fixture(scope="module")
def sphere_capture(tmp_path_factory):
    """The Lambert sphere of tests/test_data_gpu.py seen from the radius-4 shell through DISTORTED per-frame cameras, rendered by
    the float64 reference and written as a nerfstudio-format directory: PNG frames and, every fifth one, JPEG at quality 95."""
    H = W = 48
    poses = ref.shell_poses(E2E_FRAMES)
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    rows = np.stack([[focal * (1.0 + 0.01 * (i % 5)), focal * (1.03 - 0.01 * (i % 3)), W / 2 - 0.6, H / 2 + 0.3, *ref.TEST_COEFFS]
                     for i in range(E2E_FRAMES)])
    ims = np.stack([np.clip(np.rint(ref.sphere_image(poses[i], rows[i], H, W) * 255.0), 0, 255).astype(np.uint8) for i in range(E2E_FRAMES)])
    names = [f"images/frame_{i:05d}.{'jpg' if i % 5 == 4 else 'png'}" for i in range(E2E_FRAMES)]
    root = ref.write_capture(str(tmp_path_factory.mktemp("sphere") / "capture"), ims, poses, rows, names=names)
    return root, poses, rows


def _args(*argv):
    ap = trainer.build_parser()
    return ap, ap.parse_args(list(argv))


def test_train_eval_render_end_to_end_on_a_distorted_capture(sphere_capture, tmp_path):
    root, poses, rows = sphere_capture
    run = str(tmp_path / "run")
    ap, args = _args("train", "--data", root, "--out", run, "--near", "0.5", "--far", "1.5", "--primary-spacing", "uniform")
    scene, settings = trainer.load_scene(ap, args, "train")
    i_train, i_eval = ref.split_indices(E2E_FRAMES, 0.9)
    assert scene.num_images == 24 and settings == {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS}
    assert np.array_equal(scene.cameras, rows[i_train].astype(np.float32))
    assert abs(np.abs(scene.c2w[:, :, 3]).max() - 1.0) <= 0.05  # auto-scale over all 26 frames: the shell of radius 4 at about 1/4
    logs = []
    ck = trainer.train(scene, run, steps=E2E_STEPS, rays=1024, save_every=200, log_every=100, seed=0, device=DEV, model_config=_cfg(),
                       log=logs.append, near=args.near, far=args.far, primary_spacing=args.primary_spacing, data_settings=settings,
                       deterministic=True)  # a fixed reduction order: the gain below is a function of the code alone
    assert ck.endswith(f"step-{E2E_STEPS - 1:09d}.ckpt") and "near 0.5 far 1.5 primary_spacing uniform" in logs[0]
    # nerfstudio's dataparser_transforms.json, and the same record in the checkpoint
    import json

    written = json.load(open(os.path.join(run, "dataparser_transforms.json")))
    want_poses, want_transform = ref.orient_and_center(poses)
    want_scale = 1.0 / np.abs(want_poses[:, :, 3]).max()
    assert np.abs(np.array(written["transform"]) - want_transform).max() <= 1e-12 and abs(written["scale"] - want_scale) <= 1e-12
    rec = checkpoint.read_run_state(run)
    assert rec["data"] == {**settings, "transform": written["transform"], "scale": written["scale"]}
    assert (rec["near"], rec["far"], rec["primary_spacing"]) == (0.5, 1.5, "uniform") and "primary_tan" not in rec
    # eval with no data flags: the split and the normalisation come from the checkpoint
    ap, args = _args("eval", "--data", root, "--ckpt", run)
    held_out, _ = trainer.load_scene(ap, args, args.split, checkpoint.read_run_state(args.ckpt))
    want_poses[:, :, 3] *= want_scale
    assert held_out.file_paths == [f"images/frame_{i:05d}.{'jpg' if i % 5 == 4 else 'png'}" for i in i_eval] and len(i_eval) == 2
    assert np.abs(held_out.c2w - want_poses[i_eval]).max() <= 1e-6 and np.array_equal(held_out.cameras, rows[i_eval].astype(np.float32))
    init = trainer.make_model(checkpoint.config_with_planes(_cfg(), 0.5, 1.5), seed=0)
    opt0 = pkg.FusedRAdam(init.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ck0 = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "init"), 0), init, opt0, 0,
                                  checkpoint.make_run_state(0, 1024, "f32", False, DEV, **{"near": 0.5, "far": 1.5}))
    before = trainer.evaluate(held_out, ck0, device=DEV, model_config=_cfg())
    after = trainer.evaluate(held_out, run, device=DEV, model_config=_cfg())
    assert after["checkpoint"] == ck and len(after["per_image"]) == 2
    gain = after["results"]["psnr"] - before["results"]["psnr"]
    print(f"capture end to end: held-out psnr {before['results']['psnr']:.2f} -> {after['results']['psnr']:.2f} dB (gain {gain:.2f}); "
          f"bound {E2E_MIN_GAIN_DB:.2f} = half the Blender path's {E2E_BLENDER_GAIN_DB:.2f}")
    # render --data: the file's frames through their own cameras
    out = str(tmp_path / "frames")
    ap, args = _args("render", "--ckpt", run, "--out", out, "--data", root, "--split", "val", "--channels", "rgb", "depth")
    cams = trainer.resolve_render_args(ap, args)
    assert np.array_equal(cams["camera_table"], rows[i_eval].astype(np.float32)) and np.array_equal(cams["c2w"], held_out.c2w)
    res = render.render_checkpoint(args.ckpt, args.out, *render.camera_args(cams), camera_table=cams["camera_table"], channels=args.channels,
                                   model_config=_cfg(), device=DEV)
    assert os.path.isfile(os.path.join(out, "panel", "0000.png")) and len(res["frames"]) == 2
    assert res["frames"][0]["camera"] == [float(v) for v in rows[i_eval[0]].astype(np.float32)] and res["depth_range"] == [0.5, 1.5]
    # the TSDF and point-cloud exports project through one shared pinhole: a distorted capture is refused, in words
    ap, args = _args("export-pointcloud", "--ckpt", run, "--out", str(tmp_path / "c.ply"), "--data", root)
    with pytest.raises(SystemExit):
        trainer.resolve_pointcloud_args(ap, args)
    assert gain >= E2E_MIN_GAIN_DB, gain


def test_resume_is_bit_exact_across_the_new_settings_and_reciprocal_spacing_trains(sphere_capture, tmp_path):
    root, _, _ = sphere_capture
    ap, args = _args("train", "--data", root, "--out", "unused", "--train-split-fraction", "0.5", "--orientation", "none")
    scene, settings = trainer.load_scene(ap, args, "train")
    losses = {}
    kw = dict(steps=20, save_every=10, log_every=0, device=DEV, model_config=_cfg())
    a = trainer.train(scene, str(tmp_path / "a"), rays=256, seed=0, deterministic=True, primary_spacing="reciprocal", primary_tan=2.0,
                      near=0.5, far=1.5, data_settings=settings, on_step=lambda s, l: losses.__setitem__(s, l), **kw)
    assert all(math.isfinite(float(v)) for v in losses.values()) and len(losses) == 20
    model, _ = trainer.load_checkpoint(a, _cfg(), DEV)
    spec = model.sampler_uniform.spec  # the coarse sampler of the primary rays changed
    assert (spec.spacing, spec.tan, spec.num_samples) == (_abi.RSN_SPACING_RECIPROCAL, 2.0, 32)
    # resume from step 10 with nothing given: the settings, the data record and the frame come from the checkpoint
    ap, args = _args("train", "--data", root, "--out", "unused", "--resume", os.path.join(str(tmp_path / "a"), "step-000000010.ckpt"))
    again, settings_b = trainer.load_scene(ap, args, "train", checkpoint.read_run_state(args.resume))
    assert settings_b == settings and settings["train_split_fraction"] == 0.5 and settings["orientation"] == "none"
    assert np.array_equal(again.c2w, scene.c2w) and np.array_equal(again.cameras, scene.cameras) and again.num_images == 13
    logs = []
    b = trainer.train(again, str(tmp_path / "b"), resume=args.resume, data_settings=settings_b, log=logs.append, **kw)
    assert "deterministic True" in logs[0] and "near 0.5 far 1.5 primary_spacing reciprocal primary_tan 2.0" in logs[0]
    fa, fb = (torch.load(p, map_location="cpu", weights_only=False) for p in (a, b))
    assert fa["pipeline"].keys() == fb["pipeline"].keys() and all(torch.equal(fa["pipeline"][k], fb["pipeline"][k]) for k in fa["pipeline"])
    sa, sb = fa["optimizers"]["fields"]["state"], fb["optimizers"]["fields"]["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i] if isinstance(sa[i][k], torch.Tensor))
    ra, rb = fa[checkpoint.RUN_STATE_KEY], fb[checkpoint.RUN_STATE_KEY]
    assert ra.keys() == rb.keys() and all(torch.equal(ra[k], rb[k]) if isinstance(ra[k], torch.Tensor) else ra[k] == rb[k] for k in ra)
    # a capture's own starting points when nothing is said: 0.05 .. 256, reciprocal spacing with tan 1
    c = trainer.train(scene, str(tmp_path / "c"), steps=2, save_every=0, log_every=0, device=DEV, model_config=_cfg(), rays=64, data_settings=settings)
    rec = checkpoint.read_run_state(c)
    assert {k: rec[k] for k in checkpoint.RAY_KEYS} == trainer.CAPTURE_RAY_DEFAULTS
    # a scene without a camera table, run with its defaults, records none of the new keys and keeps the model's own 2 .. 6, uniform
    plain = BlenderScene.from_arrays(scene.images, scene.c2w, focal=scene.fx)
    d = trainer.train(plain, str(tmp_path / "d"), steps=2, save_every=0, log_every=0, device=DEV, model_config=_cfg(), rays=64)
    assert not {"near", "far", "primary_spacing", "primary_tan", "data"} & set(checkpoint.read_run_state(d))
    assert not os.path.exists(os.path.join(str(tmp_path / "d"), "dataparser_transforms.json"))
    model, _ = trainer.load_checkpoint(d, _cfg(), DEV)
    assert model.config.collider_params == {"near_plane": 2.0, "far_plane": 6.0} and model.sampler_uniform.spec.spacing == _abi.RSN_SPACING_UNIFORM
