"""Geometry metrics on the GPU: rsn_normal_error against the float64 reference at every size where its launch changes shape, its
fixed-order reduction, metrics.normal_error without a device-to-host read, and eval --normals end to end on the sphere toy."""
import json
import math

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, metrics, trainer
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from tests import geometry_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 1 pixel; around a wave (64) and a workgroup (256); and the first size at which a lane takes a second trip of the grid-stride loop
SIZES = (1, 63, 64, 65, 255, 256, 257, 256 * _abi.RSN_NORMAL_ERROR_MAX_GROUPS + 1)
# Worst |error_map - float64 reference| over SIZES (seed 0), measured on an MI355X by tools/geometry_report.py
# (profiles/geometry_metrics.json, "kernel_vs_fp64": 2.449e-05 degrees, at a reference angle of 141 degrees; 2.662e-05 with the
# rotation).  The bound is four times the unrotated figure: the factor covers other seeds and compiler versions.  The arithmetic
# agrees with the figure: the cross and dot products carry a few units of 2^-24 relative to |p||g|, so the angle is off by the
# order of 1e-6 rad, about 1e-4 degrees, at most; an fp32 angle near 180 degrees has a spacing of 1.5e-5 degrees by itself.
MEASURED_WORST_DEG = 2.449e-05
MAP_TOL_DEG = 4.0 * MEASURED_WORST_DEG


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_kernel(normals, acc, gt, rgba, rotation=None, want_map=True):
    """One rsn_normal_error call on host arrays -> (out float32 [4], error_map float32 [P] or None), both as numpy."""
    lib = pkg.load_library()
    P = len(normals)
    n, a, g, r, rot = _dev(normals), _dev(acc), _dev(gt), _dev(rgba), _dev(rotation)
    emap = torch.full((P,), -7.0, device=DEV) if want_map else None
    nbytes = int(lib.rsn_normal_error_workspace_bytes(P))
    ws = torch.full((nbytes // 8,), math.nan, dtype=torch.float64, device=DEV)  # its contents on entry must not matter
    out = torch.full((4,), -7.0, device=DEV)
    _abi.check(lib.rsn_normal_error(P, _abi.ptr(n), _abi.ptr(a), _abi.ptr(g), _abi.ptr(r), _abi.ptr(rot), _abi.ptr(emap), _abi.ptr(ws),
                                    nbytes, _abi.ptr(out), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if emap is None else emap.cpu().numpy()


def worst_map_error(sizes=SIZES, seed=0, rotation=None):
    """max over the sizes of max |device error map - float64 reference| in degrees, and where; tools/geometry_report.py records it."""
    worst = (0.0, None)
    for P in sizes:
        inp = ref.kernel_inputs(P, seed)
        _, emap = run_kernel(*inp, rotation=rotation)
        want = ref.normal_error(*inp, rotation=rotation)["error_map"]
        diff = np.abs(emap.astype(np.float64) - want)
        worst = max(worst, (float(diff.max()), {"n_pixels": P, "pixel": int(diff.argmax()), "reference_deg": float(want[diff.argmax()])}),
                    key=lambda t: t[0])
    return worst


def _ulps(got, want):
    """|got - want| in units of want's float32 spacing (both float32; equal NaNs count as 0)."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(got) and np.isnan(want):
        return 0.0
    return abs(float(got) - float(want)) / float(np.spacing(np.abs(want)))


@pytest.fixture(scope="module")
def cases():
    """Per size: the inputs, the reference, and one device run -- computed once and shared, never changed."""
    out = {}
    for P in SIZES:
        inp = ref.kernel_inputs(P)
        out[P] = (inp, ref.normal_error(*inp), run_kernel(*inp))
    return out


@pytest.mark.parametrize("P", SIZES)
def test_error_map_matches_float64(cases, P):
    inp, want, (out, emap) = cases[P]
    diff = np.abs(emap.astype(np.float64) - want["error_map"])
    print(f"P={P}: worst |error_map - fp64| = {diff.max():.3e} deg at pixel {diff.argmax()} (reference {want['error_map'][diff.argmax()]:.6f})")
    assert diff.max() <= MAP_TOL_DEG
    assert (emap[~want["valid"]] == 0.0).all()  # invalid pixels hold exactly 0, whatever their prediction
    # planted rows: the exact angles
    if P >= 1:
        assert emap[0] == 0.0
    if P >= 2:
        assert abs(float(emap[1]) - 180.0) <= MAP_TOL_DEG
    if P >= 3:
        assert emap[2] == np.float32(math.pi / 2) * np.float32(180.0 / math.pi)
    if P > 5:
        assert want["valid"][P - 1] and emap[P - 1] > 0.0  # the pixel of the second trip is scored
    assert out[3] == want["out"][3] and abs(out[0] - want["out"][0]) <= MAP_TOL_DEG  # a weighted mean of errors below the bound


@pytest.mark.parametrize("P", SIZES)
def test_reduction_is_the_float64_sum_of_the_devices_own_map(cases, P):
    """fp64 sums of at most 2^24 terms are exact far beyond fp32, in any order: the outputs are the fp32 roundings of the float64
    quotients formed on the host from the device's own error map, the alpha bytes and the accumulation, within 1 fp32 ulp."""
    (normals, acc, gt, rgba), want, (out, emap) = cases[P]
    host = ref.reduce(emap, want["valid"], rgba[:, 3], acc)
    for k in range(3):
        assert _ulps(out[k], np.float32(host[k])) <= 1.0, (k, out[k], host[k])
    assert out[3] == host[3] == want["valid"].sum()


@pytest.mark.parametrize("P", [65, 257, SIZES[-1]])
def test_runs_are_bit_identical_and_optional_arguments_change_nothing_else(cases, P):
    inp, _, (out, emap) = cases[P]
    out2, emap2 = run_kernel(*inp)
    assert out.tobytes() == out2.tobytes() and emap.tobytes() == emap2.tobytes()
    out3, none = run_kernel(*inp, want_map=False)
    assert none is None and out3.tobytes() == out.tobytes()
    normals, acc, gt, rgba = inp
    out4, emap4 = run_kernel(normals, None, gt, rgba)
    assert out4[2] == 0.0 and out4[[0, 1, 3]].tobytes() == out[[0, 1, 3]].tobytes() and emap4.tobytes() == emap.tobytes()


@pytest.mark.parametrize("P", [1, 257, SIZES[-1]])
def test_all_alpha_zero_gives_nan_and_zero_weight(P):
    inp = ref.kernel_inputs(P, all_alpha_zero=True)
    out, emap = run_kernel(*inp)
    assert math.isnan(out[0]) and out[1] == 0.0 and out[3] == 0.0 and (emap == 0.0).all()
    assert _ulps(out[2], np.float32(np.abs(inp[1].astype(np.float64)).mean())) <= 1.0  # the alpha error is over all pixels


@pytest.mark.parametrize("P", [257, SIZES[-1]])
def test_rotation_matches_the_rotated_reference(cases, P):
    inp, plain, _ = cases[P]
    R = ref.rotation_matrix()
    out, emap = run_kernel(*inp, rotation=R)
    want = ref.normal_error(*inp, rotation=R)
    diff = np.abs(emap.astype(np.float64) - want["error_map"])
    print(f"P={P}, rotated: worst |error_map - fp64| = {diff.max():.3e} deg")
    assert diff.max() <= MAP_TOL_DEG and abs(out[0] - want["out"][0]) <= MAP_TOL_DEG and out[3] == want["out"][3]
    assert np.abs(want["error_map"] - plain["error_map"]).max() > 1.0  # the rotation is no identity
    # validity is decided on the bytes, before the rotation
    assert np.array_equal(want["valid"], plain["valid"]) and (emap[~want["valid"]] == 0.0).all()


def test_non_finite_prediction_is_not_masked():
    normals, acc, gt, rgba = ref.kernel_inputs(257)
    normals = normals.copy()
    normals[100] = (np.nan, 0.0, 0.0)  # row 100: random inputs; make it valid
    gt[100], rgba[100, 3] = (10, 20, 240), 255
    out, emap = run_kernel(normals, acc, gt, rgba)
    assert math.isnan(out[0]) and math.isnan(emap[100]) and np.isfinite(np.delete(emap, 100)).all() and np.isfinite(out[1:]).all()
    rgba[100, 3] = 0  # the same row, not scored: it does not count
    out, emap = run_kernel(normals, acc, gt, rgba)
    assert np.isfinite(out).all() and emap[100] == 0.0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_normal_error_issues_no_device_to_host_read_and_matches_the_kernel():
    H, W = 37, 53
    normals, acc, gt, rgba = ref.kernel_inputs(H * W, seed=1)
    n, a, g, r = (_dev(normals).view(H, W, 3), _dev(acc).view(H, W, 1), _dev(gt).view(H, W, 3), _dev(rgba).view(H, W, 4))
    as_float = r.to(torch.float32) / 255.0  # what RayDataManager.image returns
    c2w = torch.cat([_dev(ref.rotation_matrix()), torch.ones(3, 1, device=DEV)], dim=1)
    metrics.normal_error(n, a, g, r)  # warm-up: the library
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = metrics.normal_error(n, a, g, r, error_map=True)
        from_float = metrics.normal_error(n, a.view(H, W), g, as_float)
        rotated = metrics.normal_error(n, None, g, r, c2w=c2w, error_map=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert set(got) == {"normal_mae", "normal_weight", "alpha_mae", "normal_pixels", "error_map"} and set(from_float) == set(got) - {"error_map"}
    assert all(got[k].shape == () and got[k].device.type == "cuda" for k in from_float) and got["error_map"].shape == (H, W)
    out, emap = run_kernel(normals, acc, gt, rgba)
    keys = ("normal_mae", "normal_weight", "alpha_mae", "normal_pixels")
    assert np.array([float(got[k]) for k in keys], np.float32).tobytes() == out.tobytes()
    assert np.array([float(from_float[k]) for k in keys], np.float32).tobytes() == out.tobytes()  # rint(a * 255) gives the bytes back
    assert got["error_map"].cpu().numpy().tobytes() == emap.reshape(H, W).tobytes()
    out_r, emap_r = run_kernel(normals, None, gt, rgba, rotation=ref.rotation_matrix())
    assert np.array([float(rotated[k]) for k in keys], np.float32).tobytes() == out_r.tobytes()
    assert rotated["error_map"].cpu().numpy().tobytes() == emap_r.reshape(H, W).tobytes()


def test_normal_error_refuses_wrong_shapes_dtypes_and_devices():
    H, W = 12, 16
    n, a = torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, 1, device=DEV)
    g, r = torch.zeros(H, W, 3, dtype=torch.uint8, device=DEV), torch.zeros(H, W, 4, dtype=torch.uint8, device=DEV)
    metrics.normal_error(n, a, g, r)
    for bad in (lambda: metrics.normal_error(n[..., :2], a, g, r), lambda: metrics.normal_error(n.double(), a, g, r),
                lambda: metrics.normal_error(n, a[:-1], g, r), lambda: metrics.normal_error(n, a.double(), g, r),
                lambda: metrics.normal_error(n, a, g.float(), r), lambda: metrics.normal_error(n, a, g[:, :-1], r),
                lambda: metrics.normal_error(n, a, g, r[..., :3]), lambda: metrics.normal_error(n, a, g, r.to(torch.int32)),
                lambda: metrics.normal_error(n, a, g.cpu(), r), lambda: metrics.normal_error(n, a, g, r.cpu()),
                lambda: metrics.normal_error(n.cpu(), a.cpu(), g.cpu(), r.cpu()),
                lambda: metrics.normal_error(n, a, g, r, c2w=torch.eye(3, device=DEV)),
                lambda: metrics.normal_error(n, a, g, r, c2w=torch.eye(4)[:3])):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ end to end
def _cfg():
    """The 4-layer, width-64, 32/32/16/16-sample model of test_data_gpu's end-to-end test."""
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                             num_reflect_importance_samples=16, base_mlp_num_layers=4, base_mlp_layer_width=64)


def sphere_scene(n, offset=0.0, normals=True):
    images, poses, focal, nrm = ref.sphere_views(n, offset=offset)
    return BlenderScene.from_arrays(images, poses, focal=focal, normals=nrm if normals else None)


def untrained_checkpoint(where):
    init = trainer.make_model(_cfg(), seed=0)
    opt0 = pkg.FusedRAdam(init.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    return trainer.save_checkpoint(trainer.checkpoint_path(str(where), 0), init, opt0, 0)


RESULT_KEYS = {k + s for k in ("psnr", "coarse_psnr", "fine_psnr", "fine_ssim", "num_rays_per_sec", "fps") for s in ("", "_std")}
PER_IMAGE_KEYS = {"image", "psnr", "coarse_psnr", "fine_psnr", "fine_ssim", "num_rays_per_sec", "fps"}
TOP_KEYS = {"experiment_name", "method_name", "checkpoint", "step", "results", "not_computed", "per_image"}
NEW_RESULT_KEYS = {"normal_mae", "normal_mae_std", "alpha_mae", "alpha_mae_std", "normal_mae_views"}


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return sphere_scene(2), untrained_checkpoint(tmp_path_factory.mktemp("geometry") / "init")


def test_eval_with_normals_end_to_end(toy, tmp_path):
    sc, ck = toy
    assert sc.normals.shape == (2, 48, 48, 3) and (sc.normals == 128).all(-1).any() and not (sc.normals == 128).all(-1).all()
    res = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), normals=True, save_images=str(tmp_path / "img"))
    json.dumps(res)  # serialisable as written by the CLI
    assert set(res) == TOP_KEYS | {"geometry"} and "level 0" in res["geometry"]["note"] and res["geometry"]["normals_space"] == "world"
    assert set(res["results"]) == RESULT_KEYS | NEW_RESULT_KEYS
    assert all(set(p) == PER_IMAGE_KEYS | {"normal_mae", "alpha_mae", "normal_weight"} for p in res["per_image"])
    r = res["results"]
    per = [p["normal_mae"] for p in res["per_image"]]
    assert r["normal_mae_views"] == 2 and r["normal_mae"] == pytest.approx(np.mean(per), abs=1e-12)
    assert r["normal_mae_std"] == pytest.approx(np.std(per, ddof=1), abs=1e-12)
    assert r["alpha_mae"] == pytest.approx(np.mean([p["alpha_mae"] for p in res["per_image"]]), abs=1e-12)
    assert all(0.0 < p["normal_mae"] < 180.0 and 0.0 <= p["alpha_mae"] <= 1.0 for p in res["per_image"])
    # normal_weight: every pixel of the toy has alpha 255, so it is the number of pixels the sphere covers
    covered = [(sc.normals[k] != 128).any(-1).sum() for k in range(2)]
    assert [p["normal_weight"] for p in res["per_image"]] == covered
    # the per-image figures are metrics.normal_error on a fresh render of the same view
    model, _ = trainer.load_checkpoint(ck, _cfg(), DEV)
    model.config.eval_num_rays_per_chunk = trainer.EVAL_CHUNK
    dm = RayDataManager(sc, DEV)
    out = model.get_outputs_for_camera_ray_bundle(dm.camera_ray_bundle(1))
    composited = (out["weights_fine"] * out["pred_normals_fine"]).sum(dim=-2)
    again = metrics.normal_error(composited, out["accumulation_fine"], dm.normal_image(1), dm.image(1))
    assert res["per_image"][1]["normal_mae"] == pytest.approx(float(again["normal_mae"]), abs=1e-9)
    assert res["per_image"][1]["alpha_mae"] == pytest.approx(float(again["alpha_mae"]), abs=1e-9)
    assert dm.normal_image(1).dtype == torch.uint8 and np.array_equal(dm.normal_image(1).cpu().numpy(), sc.normals[1])
    with pytest.raises(IndexError):
        dm.normal_image(2)
    # the panel: prediction | ground truth | error
    from PIL import Image

    with Image.open(tmp_path / "img" / "0000_normals.png") as im:
        assert im.size == (144, 48) and im.mode == "RGB"
        panel = np.asarray(im)
    assert (tmp_path / "img" / "0001_normals.png").exists() and (tmp_path / "img" / "0000_img.png").exists()
    # the middle tile is the ground truth drawn back: the map's own bytes where the sphere is (alpha 255: nothing blended in)
    assert np.abs(panel[:, 48:96].astype(int) - sc.normals[0].astype(int)).max() <= 1


def test_eval_without_normals_keeps_todays_keys(toy, tmp_path):
    sc, ck = toy
    res = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), save_images=str(tmp_path / "img"))
    assert set(res) == TOP_KEYS and set(res["results"]) == RESULT_KEYS and all(set(p) == PER_IMAGE_KEYS for p in res["per_image"])
    assert sorted(p.name for p in (tmp_path / "img").iterdir()) == ["0000_img.png", "0001_img.png"]
    with pytest.raises(ValueError, match="no normal maps"):
        RayDataManager(sphere_scene(1, normals=False), DEV).normal_image(0)
    # and the shared figures do not depend on the flag
    with_n = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), normals=True, normals_space="camera")
    for k in ("psnr", "coarse_psnr", "fine_psnr", "fine_ssim"):
        assert with_n["results"][k] == res["results"][k]
    assert with_n["geometry"]["normals_space"] == "camera"
    # world-space maps read as camera-space ones are another, worse, comparison: the flag reaches the kernel
    world = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), normals=True)
    assert with_n["results"]["normal_mae"] != world["results"]["normal_mae"]
    assert with_n["results"]["alpha_mae"] == world["results"]["alpha_mae"]


def test_multiscale_eval_scores_geometry_at_level_0_only(toy):
    sc, ck = toy
    one = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), normals=True)
    two = trainer.evaluate(sc, ck, device=DEV, model_config=_cfg(), normals=True, multiscale=2)
    assert len(two["per_image"]) == 4
    for p in two["per_image"]:
        assert ("normal_mae" in p) == ("alpha_mae" in p) == ("normal_weight" in p) == (p["level"] == 0)
    assert not [k for k in two["results"] if k.startswith(("normal_", "alpha_")) and "_x" in k]
    assert NEW_RESULT_KEYS <= set(two["results"]) and "psnr_x2" in two["results"] and "geometry" in two and "multiscale" in two
    for k in NEW_RESULT_KEYS:  # level 0 is the single-scale render: the same figures
        assert two["results"][k] == one["results"][k]


def test_cli_eval_with_normals_reads_the_maps_and_writes_the_keys(toy, tmp_path, capsys):
    """The command line end to end: the scene from disk with a custom suffix, the flags through to evaluate, the JSON on disk."""
    from PIL import Image

    from reflect_sampling_nerf_amd.data import load_blender_split

    sc, ck = toy
    root = tmp_path / "scene"
    (root / "test").mkdir(parents=True)
    frames = []
    for i in range(sc.num_images):
        Image.fromarray(sc.images[i], "RGBA").save(root / "test" / f"r_{i}.png")
        Image.fromarray(sc.normals[i], "RGB").save(root / "test" / f"r_{i}_nrm.png")
        frames.append({"file_path": f"./test/r_{i}", "transform_matrix": np.concatenate([sc.c2w[i], [[0, 0, 0, 1]]]).tolist()})
    (root / "transforms_test.json").write_text(json.dumps({"camera_angle_x": 0.6911112070083618, "frames": frames}))
    out = tmp_path / "metrics.json"
    assert trainer.main(["eval", "--data", str(root), "--ckpt", ck, "--out", str(out), "--normals", "--normals-suffix", "_nrm"]) == 0
    assert "normal_mae" in capsys.readouterr().out
    res = json.loads(out.read_text())
    loaded = load_blender_split(str(root), "test", normals=True, normals_suffix="_nrm")
    assert np.array_equal(loaded.normals, sc.normals)
    want = trainer.evaluate(loaded, ck, device=DEV, normals=True)
    assert NEW_RESULT_KEYS <= set(res["results"]) and res["geometry"] == want["geometry"]
    for k in sorted(NEW_RESULT_KEYS) + ["psnr", "fine_ssim"]:
        assert res["results"][k] == want["results"][k], k
    plain = tmp_path / "plain.json"
    assert trainer.main(["eval", "--data", str(root), "--ckpt", ck, "--out", str(plain)]) == 0
    got = json.loads(plain.read_text())
    assert set(got) == TOP_KEYS and set(got["results"]) == RESULT_KEYS and got["results"]["psnr"] == res["results"]["psnr"]
