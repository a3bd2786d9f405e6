"""GPU checks of the multi-scale data path: rsn_build_pyramid and rsn_sample_pyramid_rays against the host restatements
(tests/pyramid_reference.py) by bits, level frequencies, a host-sync-free multi-scale step, the argument errors of both C calls,
eval per scale, a bit-exact multi-scale resume, and multi-scale train -> eval end to end on an analytically rendered scene.

Shapes: N = 3 images of 48 x 80 with L = 5 levels -- not square, the last level 3 x 5 (smaller than a wave, odd width), several
workgroups at level 1, and waves of the one-launch build that straddle the boundaries between levels 2, 3 and 4."""
import json
import math

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, metrics, trainer
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from tests.data_reference import blend_white_f32, camera_rays
from tests.pyramid_reference import pyramid_flat, pyramid_level, pyramid_offsets, sample_levels_and_indices

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N, H, W = 3, 48, 80
FOCAL = 1111.1  # the Blender scenes' focal length in pixels: a pixel subtends 1e-3 rad, the regime of the pixel_area check below


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


@pytest.fixture(scope="module")
def scene():
    """uint8 RGBA noise; alpha forced to 0 in one block and to 255 in another (both ends of the blend, each covering whole boxes
    of every level); random poses; the principal point off the centre."""
    rng = np.random.default_rng(0)
    ims = rng.integers(0, 256, size=(N, H, W, 4), dtype=np.uint8)
    ims[0, :16, :32, 3] = 0
    ims[1, 16:48, 32:64, 3] = 255
    poses = np.zeros((N, 3, 4), np.float32)
    for i in range(N):
        poses[i, :, :3] = _rot(*rng.uniform(-math.pi, math.pi, 3))
        poses[i, :, 3] = rng.normal(size=3) * 3.0
    return BlenderScene.from_arrays(ims, poses, focal=FOCAL, cx=W / 2.0 - 0.7, cy=H / 2.0 + 0.4)


@pytest.fixture(scope="module")
def reference(scene):
    """The five levels' restatement, computed once: {"flat": [3825, 3], "level": {l: [N, H_l, W_l, 3]}}."""
    return {"flat": pyramid_flat(scene.images, 5), "level": {l: pyramid_level(scene.images, l) for l in range(1, 5)}}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. the pyramid
def test_every_level_equals_the_reference_bit_for_bit(scene, reference):
    dm = RayDataManager(scene, DEV, levels=5)
    got = dm.pyramid.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (3825, 3) and list(dm.level_offsets) == pyramid_offsets(N, H, W, 5)
    assert np.array_equal(_bits(got), _bits(reference["flat"]))
    assert np.array_equal(dm.image(0, 1)[:8, :16].cpu().numpy(), np.ones((8, 16, 3), np.float32))  # the alpha-0 block: exactly white
    for level in range(1, 5):
        for i in range(N):
            img = dm.image(i, level)
            assert img.shape == (H >> level, W >> level, 3) and img.dtype == torch.float32
            assert img.untyped_storage().data_ptr() == dm.pyramid.untyped_storage().data_ptr()  # a view, no copy
            assert np.array_equal(_bits(img.cpu().numpy()), _bits(reference["level"][level][i])), (level, i)
    # level 0 is what it was: the RGBA image over 255; fewer levels are a prefix of the same allocation; twice gives the same bits
    plain = RayDataManager(scene, DEV)
    assert plain.pyramid is None and torch.equal(dm.image(1), plain.image(1)) and dm.image(1).shape == (H, W, 4)
    assert torch.equal(RayDataManager(scene, DEV, levels=3).pyramid, dm.pyramid[:3600])
    assert torch.equal(RayDataManager(scene, DEV, levels=5).pyramid, dm.pyramid)
    with pytest.raises(IndexError):
        dm.image(0, 5)
    with pytest.raises(IndexError):
        plain.camera_ray_bundle(0, 1)


# ------------------------------------------------------------------------------------------------ 2. one level
def _c_sample(lib, dm, levels, R, seed, rank, step, pyramid=None):
    """rsn_sample_pyramid_rays called directly -> dict of host arrays."""
    s = dm.scene
    o, d, rgb = (torch.empty(R, 3, device=DEV) for _ in range(3))
    pa = torch.empty(R, 1, device=DEV)
    idx, lvl = torch.empty(R, 3, device=DEV, dtype=torch.int32), torch.full((R,), -1, device=DEV, dtype=torch.int32)
    _abi.check(lib.rsn_sample_pyramid_rays(s.num_images, s.height, s.width, levels, _abi.ptr(dm.images), _abi.ptr(pyramid),
                                           0 if pyramid is None else pyramid.shape[0], _abi.ptr(dm.c2w), s.fx, s.fy, s.cx, s.cy, R, seed,
                                           rank, step, _abi.ptr(o), _abi.ptr(d), _abi.ptr(pa), _abi.ptr(rgb), _abi.ptr(idx), _abi.ptr(lvl),
                                           torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return {"origins": o, "directions": d, "pixel_area": pa, "rgb": rgb, "indices": idx, "levels": lvl}


@pytest.mark.parametrize("step", [0, 17])
def test_one_level_is_byte_identical_to_the_single_scale_sampler(scene, step):
    """levels=1 through RayDataManager (the single-scale code path) and through rsn_sample_pyramid_rays itself with L = 1 and no
    pyramid: origins, directions, pixel_area, rgb and indices have the bytes of a plain RayDataManager's batch; nonzero rank."""
    R, seed, rank = 4096, 1234, 2
    plain = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=seed, rank=rank)
    rb0, b0 = plain.next_train(step)
    one = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=seed, rank=rank, levels=1)
    rb1, b1 = one.next_train(step)
    got = _c_sample(pkg.load_library(), plain, 1, R, seed, rank, step)
    assert set(b1) == {"image", "indices"} and one.pyramid is None
    for name, want, a in (("origins", rb0.origins, rb1.origins), ("directions", rb0.directions, rb1.directions),
                          ("pixel_area", rb0.pixel_area, rb1.pixel_area), ("rgb", b0["image"], b1["image"]),
                          ("indices", b0["indices"], b1["indices"])):
        assert a.dtype == want.dtype and a.shape == want.shape
        for other in (a, got[name]):
            assert np.array_equal(other.cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8)), name
    assert not bool(got["levels"].any())


# ------------------------------------------------------------------------------------------------ 3. three levels
def test_three_levels_match_the_reference_and_the_level_cameras(scene, reference):
    R, L, seed, rank, step = 4096, 3, 77, 1, 5
    dm = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=seed, rank=rank, levels=L)
    rb, b = dm.next_train(step)
    torch.cuda.synchronize()
    want_lvl, want_idx = sample_levels_and_indices(N, H, W, L, R, seed, rank, step)
    lvl, idx = b["levels"].cpu().numpy(), b["indices"].cpu().numpy()
    assert b["levels"].dtype == torch.int32 and lvl.shape == (R,) and b["indices"].dtype == torch.int32 and idx.shape == (R, 3)
    assert np.array_equal(lvl, want_lvl) and np.array_equal(idx, want_idx)
    assert np.array_equal(rb.camera_indices.cpu().numpy()[:, 0], want_idx[:, 0]) and rb.nears is None
    assert set(np.unique(lvl)) == {0, 1, 2}
    i, y, x = idx[:, 0], idx[:, 1], idx[:, 2]
    # rgb: today's fp32 blend at level 0, the pyramid's value above, by bits
    rgb = b["image"].cpu().numpy()
    want_rgb = blend_white_f32(scene.images[i, np.minimum(y, H - 1), np.minimum(x, W - 1)])
    for level in (1, 2):
        sel = lvl == level
        want_rgb[sel] = reference["level"][level][i[sel], y[sel], x[sel]]
    assert np.array_equal(_bits(rgb), _bits(want_rgb))
    # rays: the same device function as the level's camera image, so the same bits
    so, sd, sa = rb.origins.cpu().numpy(), rb.directions.cpu().numpy(), rb.pixel_area.cpu().numpy()[:, 0]
    n_checked = 0
    for level in range(L):
        for cam in range(N):
            full = dm.camera_ray_bundle(cam, level)
            assert full.origins.shape == (H >> level, W >> level, 3) and full.pixel_area.shape == (H >> level, W >> level, 1)
            fo, fd, fa = full.origins.cpu().numpy(), full.directions.cpu().numpy(), full.pixel_area.cpu().numpy()[..., 0]
            sel = (lvl == level) & (i == cam)
            assert np.array_equal(_bits(fo[y[sel], x[sel]]), _bits(so[sel])) and np.array_equal(_bits(fd[y[sel], x[sel]]), _bits(sd[sel]))
            assert np.array_equal(_bits(fa[y[sel], x[sel]]), _bits(sa[sel]))
            n_checked += int(sel.sum())
    assert n_checked == R
    # pixel_area.  With s = 2^l, pixel (y, x) of level l has its centre at the level-0 image-plane point (y0, x0) = ((y + .5) s - .5,
    # (x + .5) s - .5), and its neighbours lie s level-0 pixels away.  pixel_area = |d(p + t e_x) - d(p)| |d(p + t e_y) - d(p)| with d
    # the normalised direction through the image-plane point p = (vx, vy), e the axis and t the step: s / f at level l, 1 / f at level
    # 0.  Expanding d along an axis: |d(p + t e) - d(p)| = t |J e| (1 + k t + O(t^2)), where k = (J e . H e e) / (2 |J e|^2) belongs to
    # p and e alone, and |k| <= |p| for d = w / |w| (along the radius the angle's derivative is 1 / (1 + |p|^2) and its second
    # derivative -2 |p| / (1 + |p|^2)^2; across it the second-order term is orthogonal to J e).  So each factor's ratio is
    # s (1 + k (s - 1) / f + O((s / f)^2)) and area_l / (4^l area_0) deviates from 1 by at most 2 (s - 1) |p| / f: with f = 1111.1,
    # s <= 4 and |p| <= (40.7 + 24.4) / f = 0.0586 that is 3.2e-4, plus O((s / f)^2) = 1.3e-5 and the fp32 rounding of the device's
    # pixel_area (1e-5: test_data_gpu).  1e-3 is about three times the geometric bound; nothing here was measured first.
    s = (1 << lvl).astype(np.float64)
    _, _, area0 = camera_rays(scene.c2w[i].astype(np.float64), scene.fx, scene.fy, scene.cx, scene.cy, (y + 0.5) * s - 0.5, (x + 0.5) * s - 0.5)
    rel = np.abs(sa.astype(np.float64) / (4.0 ** lvl * area0) - 1.0)
    print("pixel_area / (4^l area_0) - 1, worst per level:", [float(rel[lvl == level].max()) for level in range(L)])
    assert rel.max() <= 1e-3, rel.max()


# ------------------------------------------------------------------------------------------------ 4. level frequencies
@pytest.mark.parametrize("levels", [3, 4, 5])
def test_levels_are_drawn_with_equal_probability(scene, levels):
    """Each level's count of R = 65536 rays within 4 sigma of R / L, sigma = sqrt(R (1/L)(1 - 1/L)) (a binomial count; the numpy
    restatement alone lies at 2.92, 2.30 and 2.58 sigma at worst for L = 3, 4, 5: test_pyramid_cpu); every index inside its level."""
    R = 65536
    dm = RayDataManager(scene, DEV, num_rays_per_batch=R, seed=3, rank=0, levels=levels)
    _, b = dm.next_train(7)
    lvl, idx = b["levels"].cpu().numpy().astype(np.int64), b["indices"].cpu().numpy()
    assert lvl.min() >= 0 and lvl.max() < levels
    counts = np.bincount(lvl, minlength=levels)
    sigma = math.sqrt(R * (1.0 / levels) * (1.0 - 1.0 / levels))
    dev = np.abs(counts - R / levels) / sigma
    print(f"L = {levels}: counts {counts.tolist()}, worst {dev.max():.2f} sigma")
    assert dev.max() <= 4.0, dev
    assert (idx >= 0).all() and (idx[:, 0] < N).all() and (idx[:, 1] < (H >> lvl)).all() and (idx[:, 2] < (W >> lvl)).all()
    assert np.array_equal(lvl, sample_levels_and_indices(N, H, W, levels, R, 3, 0, 7)[0])


# ------------------------------------------------------------------------------------------------ 5. no host sync
def _cfg():
    """The 4-layer, width-64, 32/32/16/16-sample model of test_data_gpu's end-to-end test."""
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                             num_reflect_importance_samples=16, base_mlp_num_layers=4, base_mlp_layer_width=64)


def test_multiscale_training_steps_issue_no_host_sync(scene):
    from reflect_sampling_nerf_amd.parallel import train_step

    model = trainer.make_model(_cfg(), seed=0).to(DEV).train()
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=50000)
    dm = RayDataManager(scene, DEV, num_rays_per_batch=256, seed=0, levels=3)
    for step in range(3):  # warm-up: one-time packing, allocator growth
        rb, b = dm.next_train(step)
        train_step(model, rb, b, opt, None, 60 + step)
    torch.cuda.synchronize()
    losses = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in range(3, 6):
            rb, b = dm.next_train(step)
            losses.append(train_step(model, rb, b, opt, None, 60 + step))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(math.isfinite(float(v)) for v in losses)


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors_of_both_calls_are_pinned(scene):
    """(return code, fragment of rsn_last_error()) of every refusal, each before any launch: the outputs keep their fill."""
    lib = pkg.load_library()
    dm = RayDataManager(scene, DEV, levels=5)
    R = 64
    f = torch.full((R * 10,), -7.0, device=DEV)
    idx, lvl = torch.full((R, 3), -7, device=DEV, dtype=torch.int32), torch.full((R,), -7, device=DEV, dtype=torch.int32)
    im, py, c2w = _abi.ptr(dm.images), _abi.ptr(dm.pyramid), _abi.ptr(dm.c2w)
    outs = [_abi.ptr(f[0:3 * R]), _abi.ptr(f[3 * R:6 * R]), _abi.ptr(f[6 * R:7 * R]), _abi.ptr(f[7 * R:]), _abi.ptr(idx), _abi.ptr(lvl)]

    def build(n=N, h=H, w=W, levels=5, images=im, pyramid=py, pixels=3825):
        return lib.rsn_build_pyramid(n, h, w, levels, images, pyramid, pixels, None), lib.rsn_last_error()

    def sample(n=N, h=H, w=W, levels=5, images=im, pyramid=py, pixels=3825, pose=c2w, fx=FOCAL, fy=FOCAL, rays=R, out=None):
        o = outs if out is None else [None if j == out else p for j, p in enumerate(outs)]
        return lib.rsn_sample_pyramid_rays(n, h, w, levels, images, pyramid, pixels, pose, fx, fy, 1.0, 1.0, rays, 0, 0, 0, *o, None), \
            lib.rsn_last_error()

    cases = [(build(levels=0), b"levels=0: 1 to 5"), (build(levels=6), b"levels=6: 1 to 5"),
             (build(n=0), b"n_images=0 height=48 width=80"), (build(h=40), b"height=40 width=80: levels=5 needs both divisible by 2^(levels-1) = 16"),
             (build(w=72), b"height=48 width=72: levels=5"), (build(n=65536, h=256, w=256), b"4294967296 pixels: at most 2^32 - 1"),
             (build(images=None), b"a pointer is NULL"), (build(pyramid=None), b"a pointer is NULL"),
             (build(pixels=3824), b"pyramid of 3824 pixels, 3825 needed"),
             (build(levels=0, h=40), b"levels=0"),  # the level count is checked first
             (sample(levels=0), b"levels=0: 1 to 5"), (sample(levels=6), b"levels=6: 1 to 5"),
             (sample(h=0), b"n_images=3 height=0 width=80"), (sample(h=56), b"height=56 width=80: levels=5 needs both divisible"),
             (sample(n=65536, h=256, w=256), b"at most 2^32 - 1"), (sample(rays=-1), b"n_rays=-1"), (sample(fx=0.0), b"fx=0 fy=1111.1"),
             (sample(images=None), b"a pointer is NULL"), (sample(pyramid=None), b"a pointer is NULL"), (sample(pose=None), b"a pointer is NULL"),
             (sample(pixels=100), b"pyramid of 100 pixels, 3825 needed")]
    cases += [(sample(out=j), b"a pointer is NULL") for j in range(6)]
    for n_case, ((rc, msg), want) in enumerate(cases):
        assert rc == -1 and want in msg, (n_case, rc, msg, want)
    assert sample(rays=0, images=None, pyramid=None, pose=None)[0] == 0  # no rays: nothing to do, no pointer read
    assert build(levels=1, images=None, pyramid=None, pixels=0)[0] == 0  # one level: nothing to build
    torch.cuda.synchronize()
    assert bool((f == -7.0).all()) and bool((idx == -7).all()) and bool((lvl == -7).all())


# ------------------------------------------------------------------------------------------------ the Lambert sphere
def _look_at(pos):
    back = pos / np.linalg.norm(pos)
    right = np.cross(np.array([0.0, 0.0, 1.0]), back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.concatenate([np.stack([right, up, back], 1), pos[:, None]], 1).astype(np.float32)


def _sphere_scene(n, H=48, W=48, offset=0.0):
    """The Lambert sphere of test_data_gpu._sphere_scene (radius 0.8, white background) seen from a radius-4 shell."""
    k = np.arange(n) + 0.5 + offset
    z = np.clip(0.8 * (1 - 2 * k / (n + 1)), -0.8, 0.8)
    phi = k * math.pi * (3 - math.sqrt(5))
    dirs = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], -1)
    poses = np.stack([_look_at(4.0 * d) for d in dirs])
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    light = np.array([0.5, 0.8, 0.3]) / np.linalg.norm([0.5, 0.8, 0.3])
    base = np.array([0.85, 0.35, 0.25])
    ims = []
    for p in poses:
        o, d, _ = camera_rays(p.astype(np.float64), focal, focal, W / 2, H / 2, yy, xx)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - 0.8 ** 2)
        t = -b - np.sqrt(np.clip(disc, 0, None))
        nrm = o + t[..., None] * d
        nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
        shade = 0.25 + 0.75 * np.clip(nrm @ light, 0, None)
        ims.append(np.where((disc > 0)[..., None], shade[..., None] * base, 1.0))
    return BlenderScene.from_arrays(np.stack(ims), poses, focal=focal)


def _untrained_checkpoint(where):
    init = trainer.make_model(_cfg(), seed=0)
    opt0 = pkg.FusedRAdam(init.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    return trainer.save_checkpoint(trainer.checkpoint_path(str(where), 0), init, opt0, 0)


TIMING_KEYS = ("num_rays_per_sec", "fps")  # wall-clock figures: the only entries of an eval that two runs do not share


# ------------------------------------------------------------------------------------------------ 7. eval
def test_eval_scores_every_view_at_every_scale(tmp_path):
    sc = _sphere_scene(2)
    ck = _untrained_checkpoint(tmp_path / "init")
    one = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg())
    two = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), multiscale=2)
    json.loads(json.dumps(two))  # serialisable as written by the CLI
    assert "multiscale" not in one and all("level" not in p for p in one["per_image"])
    assert two["multiscale"]["levels"] == 2 and two["multiscale"]["scales"] == [1, 2] and "mean of the per-scale means" in two["multiscale"]["note"]
    assert [(p["image"], p["level"]) for p in two["per_image"]] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    keys = [k for k in one["results"] if not k.endswith("_std")]
    assert {"psnr", "coarse_psnr", "fine_psnr", "fine_ssim"} <= set(keys)
    r1, r2 = one["results"], two["results"]
    assert set(r2) == set(r1) | {f"{k}_x{s}{e}" for k in keys for s in (1, 2) for e in ("", "_std")}
    for k in keys:
        assert math.isfinite(r2[k + "_x2"]) and math.isfinite(r2[k + "_x2_std"])
        assert r2[k] == pytest.approx(0.5 * (r2[k + "_x1"] + r2[k + "_x2"]), rel=1e-12)
        if k not in TIMING_KEYS:  # the same render of the same views: the same numbers, exactly
            assert r2[k + "_x1"] == r1[k] and r2[k + "_x1_std"] == r1[k + "_std"], k
    # the level-1 entries are get_image_metrics_and_images / metrics.ssim on the level's rays and the pyramid's ground truth
    model, _ = trainer.load_checkpoint(ck, _cfg(), DEV)
    model.config.eval_num_rays_per_chunk = trainer.EVAL_CHUNK
    dm = RayDataManager(sc, DEV, levels=2)
    for i in range(2):
        out = model.get_outputs_for_camera_ray_bundle(dm.camera_ray_bundle(i, 1))
        assert out["mid_reflect_fine"].shape == (24, 24, 3) and dm.image(i, 1).shape == (24, 24, 3)
        m, _ = model.get_image_metrics_and_images(out, {"image": dm.image(i, 1)})
        entry = two["per_image"][2 * i + 1]
        assert entry["psnr"] == pytest.approx(m["psnr"], abs=1e-9)
        assert entry["fine_ssim"] == pytest.approx(float(metrics.ssim(torch.clip(out["mid_reflect_fine"], 0, 1), dm.image(i, 1))), abs=1e-9)
    with pytest.raises(ValueError, match=r"level 3 are 6 x 6 pixels"):
        trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), multiscale=4)


def test_eval_culls_every_scale_with_one_occupancy_grid(tmp_path, monkeypatch):
    from reflect_sampling_nerf_amd import occupancy

    built = []
    inner = occupancy.build_occupancy
    monkeypatch.setattr(occupancy, "build_occupancy", lambda *a, **k: built.append(1) or inner(*a, **k))
    sc = _sphere_scene(2)
    ck = _untrained_checkpoint(tmp_path / "init")
    res = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), multiscale=2,
                           occupancy={"resolution": 32, "sigma": 0.01, "dilate": 1, "bounds": None})
    assert len(built) == 1 and "occupancy" in res and len(res["per_image"]) == 4
    assert all(math.isfinite(p["psnr"]) for p in res["per_image"])


# ------------------------------------------------------------------------------------------------ 8. resume
def _state_tensors(path):
    ck = torch.load(path, map_location="cpu", weights_only=False)
    out = {"pipeline/" + k: v for k, v in ck["pipeline"].items()}
    for i, st in ck["optimizers"]["fields"]["state"].items():
        for k in ("exp_avg", "exp_avg_sq", "step"):
            out[f"optimizer/{i}/{k}"] = torch.as_tensor(st[k])
    out["run/cuda_rng_state"], out["run/cpu_rng_state"] = ck["rsn_run"]["cuda_rng_state"], ck["rsn_run"]["cpu_rng_state"]
    return out, ck["rsn_run"]


def test_deterministic_multiscale_resume_is_bit_exact(tmp_path):
    """Four steps straight against two steps, a save, a load and two more: every model tensor, every optimiser moment and step count
    and both generator states by bits.  The resumed call is not told the level count: it comes from the checkpoint."""
    sc = _sphere_scene(6)
    kw = dict(device=DEV, model_config=_cfg(), log_every=0, save_every=0)
    a = trainer.train(sc, str(tmp_path / "a"), steps=4, rays=256, seed=0, deterministic=True, multiscale=3, log=None, **kw)
    b2 = trainer.train(sc, str(tmp_path / "b"), steps=2, rays=256, seed=0, deterministic=True, multiscale=3, log=None, **kw)
    logs = []
    b = trainer.train(sc, str(tmp_path / "b"), steps=4, resume=b2, log=logs.append, **kw)
    assert a.endswith("step-000000003.ckpt") and b2.endswith("step-000000001.ckpt") and b.endswith("step-000000003.ckpt")
    assert logs[0].endswith("steps 4 rays 256 mma f32 seed 0 deterministic True multiscale 3") and not [s for s in logs if "not bit-exact" in s]
    (ta, run_a), (tb, run_b) = _state_tensors(a), _state_tensors(b)
    assert run_a["multiscale"] == 3 and run_b["multiscale"] == 3 and _state_tensors(b2)[1]["multiscale"] == 3
    assert sorted(ta) == sorted(tb) and len([k for k in ta if k.startswith("optimizer/")]) >= 3
    assert [k for k in ta if not torch.equal(ta[k], tb[k])] == []
    # the control: a single-scale run of the same length differs (the level count does reach the batches) and records no level count
    c = trainer.train(sc, str(tmp_path / "c"), steps=4, rays=256, seed=0, deterministic=True, log=None, **kw)
    tc, run_c = _state_tensors(c)
    assert "multiscale" not in run_c and any(not torch.equal(ta[k], tc[k]) for k in ta if k.startswith("pipeline/"))


# ------------------------------------------------------------------------------------------------ 9. end to end
E2E_STEPS = 400
# Test-view PSNR per scale (reflect-fine render) of the step-0 model and after 400 multi-scale steps, measured on an MI355X:
# 1/1: 4.85 -> 9.12 dB (+4.27), 1/2: 5.00 -> 9.43 dB (+4.43), 1/4: 5.20 -> 9.95 dB (+4.75); beside a single-scale run of the same
# length: profiles/multiscale.json ("toy_scene").  The condition is a gain above zero at every scale; no larger bound is fixed:
# this is one run on a toy scene.


def test_multiscale_train_eval_end_to_end(tmp_path):
    train_scene, test_scene = _sphere_scene(24), _sphere_scene(4, offset=0.37)
    ck0 = _untrained_checkpoint(tmp_path / "init")
    ck = trainer.train(train_scene, str(tmp_path / "run"), steps=E2E_STEPS, rays=1024, save_every=0, log_every=0, seed=0, device=DEV,
                       model_config=_cfg(), log=None, multiscale=3)
    before = trainer.evaluate(test_scene, ck0, device=DEV, model_config=_cfg(), multiscale=3)["results"]
    after = trainer.evaluate(test_scene, ck, device=DEV, model_config=_cfg(), multiscale=3)
    json.dumps(after)
    assert len(after["per_image"]) == 12
    gains = {s: after["results"][f"psnr_x{s}"] - before[f"psnr_x{s}"] for s in (1, 2, 4)}
    print("multi-scale end to end: test-view psnr per scale " +
          ", ".join(f"1/{s}: {before[f'psnr_x{s}']:.2f} -> {after['results'][f'psnr_x{s}']:.2f} dB (gain {g:.2f})" for s, g in gains.items()))
    for s, g in gains.items():
        assert g > 0.0, (s, g)
