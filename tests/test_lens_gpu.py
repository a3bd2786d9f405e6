"""GPU checks of masks and fisheye cameras on the capture data path (include/rsn.h, "captures: masks and fisheye lenses"): the
live-pixel lists bit for bit against numpy.flatnonzero, rsn_sample_capture_rays_live byte for byte against rsn_sample_capture_rays
where nothing is masked and no row is a fisheye one, its indices against the Philox restatement through the reference lists, fisheye
rays against the float64 reference of tests/lens_reference.py, a host-sync-free data manager, and train -> eval -> render -> resume on
a masked, downscaled fisheye capture."""
import math
import os

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, checkpoint, data, render, trainer
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from tests import capture_reference as cref
from tests import lens_reference as ref
from tests.data_reference import blend_white_f32
from tests.pyramid_reference import pyramid_level

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N, H, W = 5, 36, 52  # 9360 pixels: several workgroups, a ragged last one, both sides divisible by 4
MASKS = ref.named_masks(N, H, W)
ULP = 2.0 ** -23


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _scene(n=N, rows=None, masks=None, seed=0, images=None):
    rng = np.random.default_rng(seed)
    ims = rng.integers(0, 256, size=(n, H, W, 4), dtype=np.uint8) if images is None else images
    poses = np.zeros((n, 3, 4), np.float32)
    for i in range(n):
        poses[i, :, :3] = _rot(*rng.uniform(-math.pi, math.pi, 3))
        poses[i, :, 3] = rng.normal(size=3) * 3.0
    cams = np.ascontiguousarray(rows, dtype=np.float32)
    return BlenderScene(images=ims, c2w=poses, fx=float(cams[0, 0]), fy=float(cams[0, 1]), cx=float(cams[0, 2]), cy=float(cams[0, 3]),
                        cameras=cams, masks=masks)


def _rows9(n=N):
    """Distorted rows with their own intrinsics at the even images, all-zero coefficients at the odd ones."""
    rows = np.stack([cref.camera_row(W, H, scale=1.0 + 0.02 * i) for i in range(n)])
    rows[1::2, 4:] = 0.0
    return rows.astype(np.float32)


def _lens_rows():
    """The rows of the float64 comparison: mild, corners beyond 90 degrees, a pixel centre on the principal point, pure equidistant,
    and a perspective row with distortion in the same table."""
    return np.stack([ref.fisheye_row(W, H), ref.fisheye_row(W, H, corner_theta_d=2.2), ref.fisheye_row(W, H, cx=20.5, cy=11.5),
                     ref.fisheye_row(W, H, coeffs=(0.0, 0.0, 0.0, 0.0)), ref.perspective_row12(W, H)]).astype(np.float32)


def _host(rb, b):
    torch.cuda.synchronize()
    out = {"origins": rb.origins, "directions": rb.directions, "pixel_area": rb.pixel_area, "image": b["image"], "indices": b["indices"]}
    if "levels" in b:
        out["levels"] = b["levels"]
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ------------------------------------------------------------------------------------------------ 1. lists
def _build(masks, levels, fill=True, poison=0x5A5A5A5A):
    """-> (counts uint32 [levels], live uint32 [capacity]) of one rsn_build_live_pixels call; capacity = the reference's total + 8,
    poisoned, so that a write past the lists' end shows."""
    lib = _abi.load_library()
    n, h, w = masks.shape
    dev_masks = torch.from_numpy(np.ascontiguousarray(masks)).to(DEV)
    ws_bytes = lib.rsn_live_pixels_workspace_bytes(n, h, w, levels)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes // 4, device=DEV, dtype=torch.int32)
    counts = torch.full((levels,), -1, device=DEV, dtype=torch.int32)
    total = sum(len(x) for x in ref.live_lists(masks, levels))
    live = torch.full((total + 8,), poison, device=DEV, dtype=torch.int32) if fill else None
    _abi.check(lib.rsn_build_live_pixels(n, h, w, levels, _abi.ptr(dev_masks), _abi.ptr(live), total if fill else 0, _abi.ptr(counts),
                                         _abi.ptr(ws), ws_bytes, torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return counts.cpu().numpy().view(np.uint32), (live.cpu().numpy().view(np.uint32) if fill else None)


def _check_lists(masks, levels):
    want = ref.live_lists(masks, levels)
    flat = np.concatenate(want)
    counted, _ = _build(masks, levels, fill=False)
    assert counted.tolist() == [len(x) for x in want]
    for poison in (0x5A5A5A5A, 0x21212121):  # a second run into a buffer poisoned otherwise repeats the first
        counts, live = _build(masks, levels, poison=poison)
        assert np.array_equal(counts, counted)
        assert live[:len(flat)].tobytes() == flat.tobytes()
        assert np.all(live[len(flat):] == np.uint32(poison))  # the capacity is the lists' length: nothing behind it is written


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("name", sorted(MASKS))
def test_live_pixel_lists_equal_flatnonzero_at_every_level(name, levels):
    _check_lists(MASKS[name], levels)


def test_live_pixel_lists_across_the_scans_chunk_boundaries():
    """More than 2 * RSN_LIVE_SCAN_CHUNK + 1 pixels at level 0: the scan's loop runs three trips and carries its total twice."""
    n, side = 5, 164
    assert n * side * side > 2 * 65536 + 1 and side % 4 == 0
    masks = (np.random.default_rng(11).random((n, side, side)) < 0.3).astype(np.uint8)
    masks[2] = 0  # a dead middle image
    masks[3, 40:120, 8:150] = 1  # and a region whose coarser levels are live
    _check_lists(masks, 3)


# ------------------------------------------------------------------------------------------------ 2. identity
@pytest.mark.parametrize("n", [1, 5])
def test_all_live_lists_and_perspective_rows_give_the_capture_samplers_bytes(n):
    rows = _rows9(n)
    rows12 = np.concatenate([rows, np.zeros((n, 3), np.float32)], axis=1)
    for levels in (1, 3):
        plain = _scene(n, rows=rows)
        masked = _scene(n, rows=rows, masks=np.ones((n, H, W), np.uint8))
        wide = _scene(n, rows=rows12)
        for R in (1, 63, 1025):
            old = RayDataManager(plain, DEV, num_rays_per_batch=R, seed=77, rank=3, levels=levels)
            via_lists = RayDataManager(masked, DEV, num_rays_per_batch=R, seed=77, rank=3, levels=levels)
            via_table = RayDataManager(wide, DEV, num_rays_per_batch=R, seed=77, rank=3, levels=levels)
            assert old.live is None and via_table.live is None and via_lists.live.numel() == sum(n * (H >> l) * (W >> l) for l in range(levels))
            assert via_table.cameras.shape == (levels, n, 12)
            for step in (0, 11):
                want = _host(*old.next_train(step))  # rsn_sample_capture_rays
                _same_bytes(want, _host(*via_lists.next_train(step)))
                _same_bytes(want, _host(*via_table.next_train(step)))
        for i in range(n):
            for level in range(levels):
                a, b = old.camera_ray_bundle(i, level), via_table.camera_ray_bundle(i, level)  # rsn_capture_rays_image / _image2
                for k in ("origins", "directions", "pixel_area"):
                    assert torch.equal(getattr(a, k), getattr(b, k)), (i, level, k)


# ------------------------------------------------------------------------------------------------ 3. indices
POISON = np.array([255, 0, 255, 255], np.uint8)


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("name", ["random30", "rectangle"])
def test_indices_match_philox_through_the_reference_lists_and_no_dead_pixel_is_drawn(name, levels):
    masks, R = MASKS["random30_blocks" if (name, levels) == ("random30", 3) else name], 4096  # random30 alone has no live level-2 pixel
    ims = np.random.default_rng(5).integers(0, 255, size=(N, H, W, 4), dtype=np.uint8)  # no live pixel has a red of 255
    ims[..., 3] = np.random.default_rng(6).integers(1, 256, size=(N, H, W), dtype=np.uint8)
    ims[masks == 0] = POISON
    sc = _scene(rows=_rows9(), masks=masks, images=ims)
    dm = RayDataManager(sc, DEV, num_rays_per_batch=R, seed=1234, rank=2, levels=levels)
    assert dm.live_counts == tuple(len(x) for x in ref.live_lists(masks, levels))
    got = _host(*dm.next_train(17))
    lvl, idx = ref.sample_through_lists(N, H, W, levels, ref.live_lists(masks, levels), R, seed=1234, rank=2, step=17)
    assert got["indices"].dtype == np.int32 and np.array_equal(got["indices"], idx)
    if levels > 1:
        assert np.array_equal(got["levels"], lvl) and len(np.unique(lvl)) == levels
    live = [ref.level_liveness(masks, l) for l in range(levels)]
    colours = [blend_white_f32(ims)] + [pyramid_level(ims, l) for l in range(1, levels)]
    for r in range(R):
        i, y, x = idx[r]
        assert live[lvl[r]][i, y, x], r  # every sampled pixel is live
        assert got["image"][r].tobytes() == colours[lvl[r]][i, y, x].tobytes(), r  # and rgb is the gather at that index
    poison = blend_white_f32(POISON[None])[0]
    assert not np.any(np.all(got["image"] == poison, axis=-1))
    at0 = lvl == 0
    assert at0.any() and np.all(ims[idx[at0, 0], idx[at0, 1], idx[at0, 2], 0] != 255)


def test_a_level_without_a_live_pixel_is_refused_at_construction():
    with pytest.raises(ValueError, match="no live pixel at level 2"):  # 30 % of the pixels: a 4 x 4 block is never all live
        RayDataManager(_scene(rows=_rows9(), masks=MASKS["random30"]), DEV, levels=3)
    RayDataManager(_scene(rows=_rows9(), masks=MASKS["last_pixel"]), DEV, levels=1)  # one live pixel is enough at one level
    with pytest.raises(ValueError, match="no live pixel at level 1"):
        RayDataManager(_scene(rows=_rows9(), masks=MASKS["last_pixel"]), DEV, levels=3)
    dm = RayDataManager(_scene(rows=_rows9(), masks=MASKS["last_pixel"]), DEV, num_rays_per_batch=64, levels=1)
    got = _host(*dm.next_train(0))
    assert np.all(got["indices"] == (N - 1, H - 1, W - 1))  # every ray lands on the one live pixel, the last of the last image
    eval_dm = RayDataManager(_scene(rows=_rows9(), masks=MASKS["last_pixel"]), DEV, levels=3, live_lists=False)  # eval: masks, no lists
    assert eval_dm.live is None and torch.equal(eval_dm.mask_image(N - 1).cpu(), torch.from_numpy(MASKS["last_pixel"][N - 1]))


# ------------------------------------------------------------------------------------------------ 4. fisheye rays against float64
def measure_against_float64():
    """Every pixel of every row of _lens_rows at levels 0 and 1, through rsn_capture_rays_image2 -> per quantity the worst share of
    its bound, 4 x the float32 restatement's error + one fp32 ulp of the value (directions: largest absolute component error, value
    1; pixel_area: relative error, one ulp relative), the errors themselves, and the number of pixels.  Each row and level has its
    own bound, from the restatement's error on its inputs; nothing of it is measured on the kernel."""
    worst = {"direction": 0.0, "pixel_area": 0.0}
    errors = {"direction": 0.0, "pixel_area_rel": 0.0, "restatement_direction": 0.0, "restatement_pixel_area_rel": 0.0}
    rows = _lens_rows()
    sc = _scene(rows=rows)
    dm = RayDataManager(sc, DEV, levels=2)
    tables = dm.cameras.cpu().numpy()
    checked, back_facing, on_axis = 0, 0, 0
    for level in range(2):
        h, w = H >> level, W >> level
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        for i in range(N):
            row32 = tables[level, i]
            assert np.array_equal(row32[:4], rows[i, :4] / np.float32(1 << level)) and np.array_equal(row32[4:], rows[i, 4:])
            row, pose = row32.astype(np.float64), sc.c2w[i].astype(np.float64)  # the reference works on the device's inputs
            o, d, area = ref.rays(pose, row, yy, xx)  # asserts the float64 inverse's residual at every pixel
            rd, ra = ref.rays_f32(sc.c2w[i], row32, yy, xx)
            rb = dm.camera_ray_bundle(i, level)
            go, gd, ga = (t.cpu().numpy() for t in (rb.origins, rb.directions, rb.pixel_area[..., 0]))
            assert np.array_equal(go, np.broadcast_to(sc.c2w[i][:, 3], (h, w, 3)))  # origins are exact
            assert np.all(np.isfinite(gd)) and np.all(np.isfinite(ga)) and ga.min() > 0.0
            cam = np.einsum("ji,...j->...i", pose[:, :3], d)
            back_facing += int((cam[..., 2] > 0.0).sum())
            on_axis += int((np.abs(cam[..., 2] + 1.0) < 1e-6).sum())  # the float32 pose is orthonormal to 1e-7; the next pixel: 1e-5
            pairs = {"direction": (np.abs(gd - d).max(), np.abs(rd - d).max(), ULP),
                     "pixel_area": ((np.abs(ga - area) / area).max(), (np.abs(ra - area) / area).max(), ULP)}
            for k, (got, restated, ulp) in pairs.items():
                bound = 4.0 * restated + ulp
                assert restated <= bound  # the reference alone stays inside it
                worst[k] = max(worst[k], got / bound)
                name = k + "_rel" if k == "pixel_area" else k
                errors[name] = max(errors[name], got)
                errors["restatement_" + name] = max(errors["restatement_" + name], restated)
            checked += h * w
    assert back_facing > 0 and on_axis >= 1  # the beyond-90 row looks backwards at its corners; one pixel looks down the axis
    return worst, errors, checked


def test_fisheye_rays_match_float64_within_four_times_the_float32_restatements_error_plus_an_ulp():
    worst, errors, checked = measure_against_float64()
    print(f"lens rays vs float64 over {checked} pixels: share of the bound (4 x the float32 restatement's error + 1 ulp) "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + "; errors " + ", ".join(f"{k} {v:.3e}" for k, v in errors.items()))
    for k, share in worst.items():
        assert share <= 1.0, (k, share)


def test_sampled_fisheye_rays_are_the_whole_view_calls_bits_at_every_level():
    levels, R = 3, 4096
    sc = _scene(rows=_lens_rows(), masks=MASKS["random30_blocks"])
    dm = RayDataManager(sc, DEV, num_rays_per_batch=R, seed=9, rank=1, levels=levels)
    got = _host(*dm.next_train(5))
    tables = dm.cameras.cpu().numpy()
    assert all(np.array_equal(tables[l, :, :4], tables[0, :, :4] / np.float32(1 << l)) for l in range(levels))  # the row's over 2^l
    views = {(i, l): dm.camera_ray_bundle(i, l) for i in range(N) for l in range(levels)}
    views = {k: tuple(getattr(v, n).cpu().numpy() for n in ("origins", "directions", "pixel_area")) for k, v in views.items()}
    assert len({(int(i), int(l)) for i, l in zip(got["indices"][:, 0], got["levels"])}) == N * levels
    for r in range(R):
        i, y, x = (int(v) for v in got["indices"][r])
        o, d, pa = views[(i, int(got["levels"][r]))]
        assert o[y, x].tobytes() == got["origins"][r].tobytes() and d[y, x].tobytes() == got["directions"][r].tobytes(), r
        assert pa[y, x].tobytes() == got["pixel_area"][r].tobytes(), r
    # the float64 reference at the sampled pixels, through the sampler
    worst = 0.0
    for i in range(N):
        for l in range(levels):
            at = (got["indices"][:, 0] == i) & (got["levels"] == l)
            y, x = got["indices"][at, 1], got["indices"][at, 2]
            _, d, area = ref.rays(sc.c2w[i].astype(np.float64), tables[l, i].astype(np.float64), y, x)
            rd, ra = ref.rays_f32(sc.c2w[i], tables[l, i], y, x)
            worst = max(worst, np.abs(got["directions"][at] - d).max() / (4.0 * np.abs(rd - d).max() + ULP),
                        (np.abs(got["pixel_area"][at, 0] - area) / area).max() / (4.0 * (np.abs(ra - area) / area).max() + ULP))
    assert worst <= 1.0, worst


# ------------------------------------------------------------------------------------------------ 5. data manager
def test_data_manager_on_a_written_masked_fisheye_capture_issues_no_host_sync(tmp_path):
    rows = _lens_rows().astype(np.float64)
    sc = _scene(rows=rows, masks=MASKS["rectangle"])
    root = ref.write_lens_capture(str(tmp_path / "capture"), sc.images, sc.c2w, rows, masks={i: sc.masks[i] for i in range(N)})
    loaded = data.load_nerfstudio_split(root, "train", eval_mode="all", orientation="none", center="none", auto_scale=False, masks=True, fisheye=True)
    assert np.array_equal(loaded.cameras, sc.cameras) and np.array_equal(loaded.c2w, sc.c2w) and np.array_equal(loaded.images, sc.images)
    assert np.array_equal(loaded.masks, sc.masks)
    for levels in (1, 3):
        dm = RayDataManager(loaded, DEV, num_rays_per_batch=1025, seed=5, levels=levels)
        want = _host(*RayDataManager(sc, DEV, num_rays_per_batch=1025, seed=5, levels=levels).next_train(3))
        dm.next_train(0), dm.camera_ray_bundle(0, levels - 1)  # warm-up: allocator growth
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            rb, b = dm.next_train(3)
            views = [dm.camera_ray_bundle(i, level) for i in (0, 4) for level in range(levels)]
            mask = dm.mask_image(4)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        _same_bytes(want, _host(rb, b))
        assert mask.data_ptr() == dm.masks[4].data_ptr() and mask.shape == (H, W)
        assert bool(torch.isfinite(rb.directions).all()) and all(bool(torch.isfinite(v.pixel_area).all()) for v in views)


def test_a_capture_with_neither_masks_nor_fisheye_makes_the_old_calls(tmp_path):
    lib = _abi.load_library()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    sc = _scene(rows=_rows9())
    root = ref.write_lens_capture(str(tmp_path / "capture"), sc.images, sc.c2w, sc.cameras.astype(np.float64))
    loaded = data.load_nerfstudio_split(root, "train", eval_mode="all", orientation="none", center="none", auto_scale=False, masks=True, fisheye=True)
    assert loaded.masks is None and loaded.cameras.shape == (N, 9)
    R = 1025
    for levels in (1, 3):
        dm = RayDataManager(loaded, DEV, num_rays_per_batch=R, seed=9, rank=1, levels=levels)
        assert dm.live is None and dm.masks is None
        rb, b = dm.next_train(4)
        flat = torch.empty(R * 10, device=DEV, dtype=torch.float32)
        o, d, pa, rgb = flat[0:3 * R].view(R, 3), flat[3 * R:6 * R].view(R, 3), flat[6 * R:7 * R].view(R, 1), flat[7 * R:10 * R].view(R, 3)
        both = torch.empty(R * 4, device=DEV, dtype=torch.int32)
        idx, lvl = both[:3 * R].view(R, 3), both[3 * R:]
        _abi.check(lib.rsn_sample_capture_rays(N, H, W, levels, _abi.ptr(dm.images), _abi.ptr(dm.pyramid), dm.pyramid.shape[0] if levels > 1 else 0,
                                               _abi.ptr(dm.c2w), _abi.ptr(dm.cameras), R, 9, 1, 4, _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa),
                                               _abi.ptr(rgb), _abi.ptr(idx), _abi.ptr(lvl), stream))
        want = {"origins": o, "directions": d, "pixel_area": pa, "image": rgb, "indices": idx}
        if levels > 1:
            want["levels"] = lvl
        torch.cuda.synchronize()
        _same_bytes({k: v.cpu().numpy() for k, v in want.items()}, _host(rb, b))
        assert set(b) == ({"image", "indices", "levels"} if levels > 1 else {"image", "indices"})


# ------------------------------------------------------------------------------------------------ 6. end to end
E2E_STEPS = 400
E2E_FRAMES = 26  # the 0.9 fraction split trains on 24 of them and holds 2 out
# This test's own deterministic run on an MI355X gains E2E_MEASURED_GAIN_DB of held-out PSNR over the live pixels in E2E_STEPS steps
# (tools/lens_report.py measures it; profiles/capture_lens.json records it).  The bound is half of that gain, as the distorted
# capture's test sizes its own.
# Measured: 5.27 -> 6.03 dB after 400 steps (and 6.97 dB after 800; after 200 the PSNR has not yet left its starting value).
E2E_MEASURED_GAIN_DB = 0.7565
E2E_MIN_GAIN_DB = 0.5 * E2E_MEASURED_GAIN_DB


def _cfg():
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                              num_reflect_importance_samples=16, base_mlp_num_layers=4, base_mlp_layer_width=64)


def write_masked_fisheye_sphere(root):
    """The Lambert sphere of tests/test_data_gpu.py seen from the radius-4 shell through per-frame FISHEYE cameras, rendered by the
    float64 reference at 48 x 48; the lower third of every image is poisoned with magenta and masked out; written as images_2 /
    masks_2 of a capture whose transforms.json describes the 96 x 96 set (which is not written: nothing reads it)."""
    S = 48
    poses = cref.shell_poses(E2E_FRAMES)
    rows = np.stack([ref.fisheye_row(S, S, coeffs=(-0.3, 0.05, -0.01, 0.002), corner_theta_d=0.45 + 0.005 * (i % 5), cx=S / 2 - 0.6, cy=S / 2 + 0.3)
                     for i in range(E2E_FRAMES)])
    ims = np.stack([np.clip(np.rint(ref.fisheye_sphere_image(poses[i], rows[i], S, S) * 255.0), 0, 255).astype(np.uint8) for i in range(E2E_FRAMES)])
    masks = np.ones((E2E_FRAMES, S, S), np.uint8)
    masks[:, 2 * S // 3:] = 0
    ims[masks == 0] = (255, 0, 255)
    ref.write_lens_capture(root, ims, poses, rows, masks={i: masks[i] for i in range(E2E_FRAMES)}, image_dir="images_2", mask_dir="masks_2",
                           declared_scale=2)
    return root, poses, rows, masks


@pytest.fixture(scope="module")
def masked_fisheye_sphere(tmp_path_factory):
    return write_masked_fisheye_sphere(str(tmp_path_factory.mktemp("lens") / "capture"))


def _args(*argv):
    ap = trainer.build_parser()
    return ap, ap.parse_args(list(argv))


def run_end_to_end(root, rows, masks, out_dir, steps=None):
    """train --downscale-factor 2 -> eval (before and after) -> render --data; -> (the numbers, the checkpoint)."""
    run, steps = os.path.join(out_dir, "run"), E2E_STEPS if steps is None else steps
    ap, args = _args("train", "--data", root, "--out", run, "--near", "0.5", "--far", "1.5", "--primary-spacing", "uniform", "--downscale-factor", "2")
    scene, settings = trainer.load_scene(ap, args, "train")
    i_train, i_eval = cref.split_indices(E2E_FRAMES, 0.9)
    assert scene.num_images == 24 and settings == {"format": "nerfstudio", **trainer.CAPTURE_DATA_DEFAULTS, "downscale_factor": 2}
    assert scene.images.shape == (24, 48, 48, 4) and np.array_equal(scene.cameras, rows[i_train].astype(np.float32)) and np.array_equal(scene.masks, masks[i_train])
    ck = trainer.train(scene, run, steps=steps, rays=1024, save_every=100, log_every=0, seed=0, device=DEV, model_config=_cfg(),
                       near=args.near, far=args.far, primary_spacing=args.primary_spacing, data_settings=settings, deterministic=True)
    rec = checkpoint.read_run_state(run)
    assert rec["data"]["downscale_factor"] == 2
    # eval with no data flags: the split, the normalisation and the downscale factor come from the checkpoint
    ap, args = _args("eval", "--data", root, "--ckpt", run)
    held_out, _ = trainer.load_scene(ap, args, args.split, checkpoint.read_run_state(args.ckpt))
    assert held_out.images.shape == (2, 48, 48, 4) and np.array_equal(held_out.cameras, rows[i_eval].astype(np.float32)) and held_out.masks is not None
    init = trainer.make_model(checkpoint.config_with_planes(_cfg(), 0.5, 1.5), seed=0)
    opt0 = pkg.FusedRAdam(init.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ck0 = trainer.save_checkpoint(trainer.checkpoint_path(os.path.join(out_dir, "init"), 0), init, opt0, 0,
                                  checkpoint.make_run_state(0, 1024, "f32", False, DEV, **{"near": 0.5, "far": 1.5}))
    before = trainer.evaluate(held_out, ck0, device=DEV, model_config=_cfg())
    after = trainer.evaluate(held_out, run, device=DEV, model_config=_cfg())
    assert after["checkpoint"] == ck and len(after["per_image"]) == 2
    for res in (before, after):
        assert {"psnr", "psnr_masked", "psnr_masked_std", "fine_ssim"} <= set(res["results"]) and all("psnr_masked" in p for p in res["per_image"])
    # psnr_masked is the PSNR of the live pixels: with every pixel live it is psnr itself, and the squared errors of a mask and of
    # its complement add up to the whole image's (the renders of one checkpoint do not depend on the masks)
    live = held_out.masks.copy()
    mse = lambda res, key: np.array([10.0 ** (-p[key] / 10.0) for p in res["per_image"]])  # noqa: E731
    held_out.masks = np.ones_like(live)
    whole = trainer.evaluate(held_out, run, device=DEV, model_config=_cfg())
    assert np.allclose(mse(whole, "psnr_masked"), mse(whole, "psnr"), rtol=1e-4) and np.allclose(mse(whole, "psnr"), mse(after, "psnr"), rtol=1e-4)
    held_out.masks = 1 - live
    rest = trainer.evaluate(held_out, run, device=DEV, model_config=_cfg())
    n_live = live.reshape(2, -1).sum(axis=1) / live[0].size
    assert np.allclose(mse(after, "psnr_masked") * n_live + mse(rest, "psnr_masked") * (1.0 - n_live), mse(after, "psnr"), rtol=1e-4)
    held_out.masks = None
    assert "psnr_masked" not in trainer.evaluate(held_out, run, device=DEV, model_config=_cfg(), max_images=1)["results"]  # without masks: unchanged
    out = os.path.join(out_dir, "frames")
    ap, args = _args("render", "--ckpt", run, "--out", out, "--data", root, "--split", "val", "--channels", "rgb")
    cams = trainer.resolve_render_args(ap, args)
    assert np.array_equal(cams["camera_table"], rows[i_eval].astype(np.float32)) and (cams["width"], cams["height"]) == (48, 48)
    res = render.render_checkpoint(args.ckpt, args.out, *render.camera_args(cams), camera_table=cams["camera_table"], channels=args.channels,
                                   model_config=_cfg(), device=DEV)
    assert os.path.isfile(os.path.join(out, "panel", "0000.png")) and len(res["frames"]) == 2 and len(res["frames"][0]["camera"]) == 12
    numbers = {"steps": steps, "psnr_masked_before": before["results"]["psnr_masked"], "psnr_masked_after": after["results"]["psnr_masked"],
               "psnr_before": before["results"]["psnr"], "psnr_after": after["results"]["psnr"]}
    numbers["gain_db"] = numbers["psnr_masked_after"] - numbers["psnr_masked_before"]
    return numbers, ck


def test_train_eval_render_end_to_end_on_a_masked_downscaled_fisheye_capture(masked_fisheye_sphere, tmp_path):
    root, _, rows, masks = masked_fisheye_sphere
    numbers, _ = run_end_to_end(root, rows, masks, str(tmp_path))
    print(f"lens end to end: held-out psnr over live pixels {numbers['psnr_masked_before']:.2f} -> {numbers['psnr_masked_after']:.2f} dB "
          f"(gain {numbers['gain_db']:.3f}); bound {E2E_MIN_GAIN_DB:.3f} = half of the measured {E2E_MEASURED_GAIN_DB}")
    assert numbers["gain_db"] >= E2E_MIN_GAIN_DB, numbers


def test_resume_is_bit_exact_with_masks_fisheye_rows_and_a_downscale_factor(masked_fisheye_sphere, tmp_path):
    root = masked_fisheye_sphere[0]
    ap, args = _args("train", "--data", root, "--out", "unused", "--downscale-factor", "2", "--near", "0.5", "--far", "1.5")
    scene, settings = trainer.load_scene(ap, args, "train")
    kw = dict(steps=20, save_every=10, log_every=0, device=DEV, model_config=_cfg())
    a = trainer.train(scene, str(tmp_path / "a"), rays=256, seed=0, deterministic=True, near=0.5, far=1.5, data_settings=settings, multiscale=2, **kw)
    # resume from step 10 with nothing given: the downscale factor comes from the checkpoint, the lists from the masks
    ap, args = _args("train", "--data", root, "--out", "unused", "--resume", os.path.join(str(tmp_path / "a"), "step-000000010.ckpt"))
    again, settings_b = trainer.load_scene(ap, args, "train", checkpoint.read_run_state(args.resume))
    assert settings_b == settings and settings["downscale_factor"] == 2
    assert np.array_equal(again.images, scene.images) and np.array_equal(again.masks, scene.masks) and np.array_equal(again.cameras, scene.cameras)
    b = trainer.train(again, str(tmp_path / "b"), resume=args.resume, data_settings=settings_b, **kw)
    fa, fb = (torch.load(p, map_location="cpu", weights_only=False) for p in (a, b))
    assert fa["pipeline"].keys() == fb["pipeline"].keys() and all(torch.equal(fa["pipeline"][k], fb["pipeline"][k]) for k in fa["pipeline"])
    sa, sb = fa["optimizers"]["fields"]["state"], fb["optimizers"]["fields"]["state"]
    assert all(torch.equal(sa[i][k], sb[i][k]) for i in sa for k in sa[i] if isinstance(sa[i][k], torch.Tensor))
    ra, rb = fa[checkpoint.RUN_STATE_KEY], fb[checkpoint.RUN_STATE_KEY]
    assert ra.keys() == rb.keys() and all(torch.equal(ra[k], rb[k]) if isinstance(ra[k], torch.Tensor) else ra[k] == rb[k] for k in ra)
