"""GPU checks of the render path: rsn_visualize against the fp64 restatement of include/rsn.h (tests/visualize_reference.py) --
every kind at shapes of one pixel, of a few, and of more than one workgroup with a partial last one, as a whole image and as a
tile inside a wider row, special values, the colour table -- the rays of an arbitrary pose, render_path end to end on a small
random model without a host synchronisation, and the `render` command from a checkpoint to PNG files.

The rule of every byte comparison (visualize_reference.check): equal to the reference, except where the reference itself says
that a value about to be truncated lies within 1e-4 of an integer; there either neighbour is right."""
import json
import math
import os

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, ops, render, trainer
from reflect_sampling_nerf_amd._abi import check, ptr
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from tests import visualize_reference as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FILL = 0xA5


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def device_draw(kind, x, alpha, lo, hi, lut, height, width, pitch, x0, out=None):
    """One rsn_visualize call through the C ABI into a panel pre-filled with FILL (or into `out`); -> (numpy [H,pitch,3], out)."""
    lib = _abi.load_library()
    if out is None:
        out = torch.full((height, pitch, 3), FILL, device=DEV, dtype=torch.uint8)
    xd, ad, ld = _dev(x), _dev(alpha), _dev(lut)
    check(lib.rsn_visualize(height, width, kind, ptr(xd), ptr(ad), float(lo), float(hi), ptr(ld), ptr(out), pitch, x0, ops._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), out


def assert_tile(panel, x0, width, want, what):
    """The tile [x0, x0 + width) obeys the rule against want = expected(...); every byte outside it is still FILL."""
    tile = panel[:, x0:x0 + width].reshape(-1, 3)
    err = ref.check(tile, *want)
    assert err is None, f"{what}: {err}"
    outside = np.ones(panel.shape[:2], dtype=bool)
    outside[:, x0:x0 + width] = False
    assert np.all(panel[outside] == FILL), f"{what}: a byte outside the tile was written"


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", [ref.RGB, ref.UNIT, ref.GRAY, ref.LUT], ids=["rgb", "unit", "gray", "lut"])
def test_every_kind_shape_and_tile_position(kind, shape):
    h, w = shape
    lut = render.TURBO if kind == ref.LUT else None
    lo, hi = ref.RANGE
    for with_alpha in (False, True):
        x, alpha = ref.random_case(kind, h, w, with_alpha)
        want = ref.expected(kind, x, alpha, lo, hi, lut)
        assert ref.ambiguous_pixels(want[1]) <= ref.MAX_AMBIGUOUS_SHARE * h * w
        for tile in ref.TILES:
            pitch, x0 = ref.tile_geometry(w, tile)
            panel, _ = device_draw(kind, x, alpha, lo, hi, lut, h, w, pitch, x0)
            assert_tile(panel, x0, w, want, f"kind {kind} {h}x{w} alpha {with_alpha} {tile}")


@pytest.mark.parametrize("kind", [ref.RGB, ref.UNIT, ref.GRAY, ref.LUT], ids=["rgb", "unit", "gray", "lut"])
def test_special_values_are_exact(kind):
    """NaN, the infinities, -0.0, values beyond both ends and on them, in x and in alpha: no byte of these cases is ambiguous
    (test_render_path_cpu asserts that), so the device bytes are the reference's; where alpha is 0, negative or NaN the pixel is
    white whatever x holds."""
    x, alpha = ref.special_values(kind)
    n = len(x)
    lo, hi = ref.SPECIAL_RANGE
    for lut in ((render.TURBO, ref.ramp_lut()) if kind == ref.LUT else (None,)):
        want = ref.expected(kind, x, alpha, lo, hi, lut)
        assert not want[1].any()
        panel, _ = device_draw(kind, x, alpha, lo, hi, lut, 1, n, n + 5, 2)
        got = panel[:, 2:2 + n].reshape(n, 3)
        assert np.array_equal(got, want[0]), np.argwhere(got != want[0])[:4]
        with np.errstate(invalid="ignore"):
            clear = np.isnan(alpha) | (alpha <= 0)
        assert clear.any() and np.all(got[clear] == 255)
        # without alpha: the same x, fully covered
        want = ref.expected(kind, x, None, lo, hi, lut)
        assert not want[1].any()
        panel, _ = device_draw(kind, x, None, lo, hi, lut, 1, n, n, 0)
        assert np.array_equal(panel.reshape(n, 3), want[0])


def test_lut_with_a_ramp_table_is_gray_and_turbo_matches_the_reference():
    """lut[k] = k/255 in all channels: the LUT kind draws floor(t*255), the GRAY kind round(t*255); on inputs t*255 = k + f with f in
    [0.1, 0.4] both are k, away from either truncation point, so the two kinds agree byte for byte (no alpha: over() is the
    identity at full coverage, and both stay exact).  Every entry below the last is hit; the last one by t = 1 further down."""
    rng = np.random.default_rng(11)
    k = np.concatenate([np.arange(255), rng.integers(0, 255, size=214)])
    x = ((k + rng.uniform(0.1, 0.4, size=k.size)) / 255.0).astype(np.float32)
    h, w = 7, 67
    assert x.size == h * w
    want_gray = ref.expected(ref.GRAY, x, None, 0.0, 1.0)
    want_lut = ref.expected(ref.LUT, x, None, 0.0, 1.0, ref.ramp_lut())
    assert not want_gray[1].any() and not want_lut[1].any() and np.array_equal(want_gray[0], want_lut[0])
    assert np.array_equal(want_gray[0][:, 0], k.astype(np.uint8))
    gray, _ = device_draw(ref.GRAY, x, None, 0.0, 1.0, None, h, w, w, 0)
    lut, _ = device_draw(ref.LUT, x, None, 0.0, 1.0, ref.ramp_lut(), h, w, w, 0)
    assert np.array_equal(gray, lut) and np.array_equal(gray.reshape(-1, 3), want_gray[0])
    # the turbo table itself, every entry: t*255 = k + 0.5, accumulation as alpha
    t = ((np.arange(256) + 0.5) / 255.0).clip(0, 1).astype(np.float32)
    t[255] = 1.0
    x = (2.0 + 4.0 * t.astype(np.float64)).astype(np.float32)
    alpha = rng.uniform(0.0, 1.0, size=256).astype(np.float32)
    want = ref.expected(ref.LUT, x, alpha, 2.0, 6.0, render.TURBO)
    panel, _ = device_draw(ref.LUT, x, alpha, 2.0, 6.0, render.TURBO, 4, 64, 64, 0)
    err = ref.check(panel.reshape(-1, 3), *want)
    assert err is None, err
    full = ref.expected(ref.LUT, x, None, 2.0, 6.0, render.TURBO)
    panel, _ = device_draw(ref.LUT, x, None, 2.0, 6.0, render.TURBO, 4, 64, 64, 0)
    assert ref.check(panel.reshape(-1, 3), *full) is None
    assert np.array_equal(full[0][:255], np.floor(render.TURBO[:255].astype(np.float64) * 255.0 + 0.5).astype(np.uint8))
    # the device copy render_path uses is this table
    assert np.array_equal(render.turbo_lut(DEV).cpu().numpy(), render.TURBO) and render.turbo_lut(DEV) is render.turbo_lut("cuda:0")


def test_two_tiles_of_one_panel_and_overwriting():
    h, w = 5, 9
    pitch = 2 * w + 3
    xa, aa = ref.random_case(ref.RGB, h, w, True)
    xb, _ = ref.random_case(ref.GRAY, h, w, False)
    wa, wb = ref.expected(ref.RGB, xa, aa), ref.expected(ref.GRAY, xb, None, 0.0, 1.0)
    _, out = device_draw(ref.RGB, xa, aa, 0.0, 1.0, None, h, w, pitch, 0)
    panel, out = device_draw(ref.GRAY, xb, None, 0.0, 1.0, None, h, w, pitch, w + 3, out=out)
    assert ref.check(panel[:, :w].reshape(-1, 3), *wa) is None
    assert ref.check(panel[:, w + 3:].reshape(-1, 3), *wb) is None
    assert np.all(panel[:, w:w + 3] == FILL)
    # a second call on the first tile overwrites all of it and nothing else
    xc, _ = ref.random_case(ref.UNIT, h, w, False)
    wc = ref.expected(ref.UNIT, xc, None)
    panel2, _ = device_draw(ref.UNIT, xc, None, 0.0, 1.0, None, h, w, pitch, 0, out=out)
    assert ref.check(panel2[:, :w].reshape(-1, 3), *wc) is None
    assert np.array_equal(panel2[:, w:], panel[:, w:])
    # through the python wrapper: the same bytes
    out3 = torch.full((h, pitch, 3), FILL, device=DEV, dtype=torch.uint8)
    render.visualize(_dev(xc).view(h, w, 3), ref.UNIT, out3, 0)
    render.visualize(_dev(xb).view(h, w), ref.GRAY, out3, w + 3, None, 0.0, 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(out3.cpu().numpy(), panel2)


def test_camera_rays_of_a_dataset_pose_are_the_data_managers():
    rng = np.random.default_rng(2)
    H, W = 6, 9
    poses = render.orbit_path(2, (0.1, -0.2, 0.3), 3.5, 25.0, 40.0)
    scene = BlenderScene.from_arrays(rng.integers(0, 256, size=(2, H, W, 4), dtype=np.uint8), poses, focal=11.3, cx=W / 2.0 - 0.3,
                                     cy=H / 2.0 + 0.2)
    dm = RayDataManager(scene, DEV)
    lib = _abi.load_library()
    for i in range(2):
        rb = render.camera_rays(scene.c2w[i], H, W, scene.fx, scene.fy, scene.cx, scene.cy, DEV)
        on_dev = render.camera_rays(dm.c2w[i], H, W, scene.fx, scene.fy, scene.cx, scene.cy, DEV)
        want = dm.camera_ray_bundle(i)
        # ... and the launch itself, as the data manager issued it before it shared this function
        o, d, pa = torch.empty(H, W, 3, device=DEV), torch.empty(H, W, 3, device=DEV), torch.empty(H, W, 1, device=DEV)
        check(lib.rsn_camera_rays_image(H, W, ptr(dm.c2w[i]), scene.fx, scene.fy, scene.cx, scene.cy, ptr(o), ptr(d), ptr(pa),
                                        ops._stream()))
        torch.cuda.synchronize()
        assert rb.origins.shape == (H, W, 3) and rb.directions.shape == (H, W, 3) and rb.pixel_area.shape == (H, W, 1)
        for got in (rb, on_dev, want):
            for a, b in ((got.origins, o), (got.directions, d), (got.pixel_area, pa)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert bool((want.camera_indices == i).all()) and want.camera_indices.shape == (H, W, 1)


# ---------------------------------------------------------------------------------------------- model -> panels
ALL_CHANNELS = tuple(render.CHANNELS)
ORBIT_RADIUS = 4.0  # cameras on the collider's sphere of interest; with it the small model reflects some rays and not others


@pytest.fixture(scope="module")
def small_model():
    """The model of test_chunked_eval_image_issues_no_device_to_host_read: 4 x 64 field, 16 / 16 / 8 / 8 samples, chunk 64."""
    torch.manual_seed(4)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=16, num_importance_samples=16, num_reflect_coarse_samples=8,
                                            num_reflect_importance_samples=8, base_mlp_num_layers=4, base_mlp_layer_width=64,
                                            eval_num_rays_per_chunk=64)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 1.5
    return cfg, model.to(DEV).eval()


def expected_panel_check(model, pose, H, W, intr, channels, depth_range, panel):
    """The panel [H, C*W, 3] against the reference applied to the model's own outputs for the same rays; -> the mask count."""
    out = model.get_outputs_for_camera_ray_bundle(render.camera_rays(pose, H, W, *intr, DEV))
    for c, name in enumerate(channels):
        ch = render.CHANNELS[name]
        x = render.channel_tensor(out, ch.source).cpu().numpy()
        alpha = None if ch.alpha is None else render.channel_tensor(out, ch.alpha).cpu().numpy().reshape(-1)
        lo, hi = depth_range if ch.lo is None else (ch.lo, ch.hi)
        x = x.reshape(-1, 3) if ch.kind in (ref.RGB, ref.UNIT) else x.reshape(-1)
        want = ref.expected(ch.kind, x, alpha, lo, hi, render.TURBO if ch.kind == ref.LUT else None)
        err = ref.check(panel[:, c * W:(c + 1) * W].reshape(-1, 3), *want)
        assert err is None, f"{name}: {err}"
    return int(out["mask"].sum())


def test_render_path_end_to_end_without_a_host_sync(small_model):
    _, model = small_model
    H, W = 10, 33
    intr = render.pinhole(W, H, 0.7)
    poses = render.orbit_path(2, (0.0, 0.0, 0.0), ORBIT_RADIUS, 20.0)
    depth_range = (0.3, 0.42)  # around the depths this random model renders (its surface sits right in front of every camera)
    render.render_path(model, poses[:1], H, W, *intr, ALL_CHANNELS, depth_range)  # warm-up: packed weights, the table, side streams
    torch.cuda.synchronize()
    seen = []
    torch.cuda.set_sync_debug_mode("error")
    try:
        render.render_path(model, poses, H, W, *intr, ALL_CHANNELS, depth_range, lambda i, a: seen.append((i, a.copy())))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert [i for i, _ in seen] == [0, 1]
    masked = []
    for i, panel in seen:
        assert panel.shape == (H, len(ALL_CHANNELS) * W, 3) and panel.dtype == np.uint8
        masked.append(expected_panel_check(model, poses[i], H, W, intr, ALL_CHANNELS, depth_range, panel))
    print(f"reflected rays per frame: {masked} of {H * W}")
    assert any(0 < m < H * W for m in masked)
    assert not np.array_equal(seen[0][1], seen[1][1])
    # a second run, this time collecting: the same bytes; and as separate images, the panel's tiles
    again = render.render_path(model, poses, H, W, *intr, ALL_CHANNELS, depth_range)
    assert len(again) == 2 and all(np.array_equal(a, s[1]) for a, s in zip(again, seen))
    tiles = render.render_path(model, poses, H, W, *intr, ALL_CHANNELS, depth_range, panel=False)
    for t, (_, panel) in zip(tiles, seen):
        assert t.shape == (len(ALL_CHANNELS), H, W, 3)
        assert np.array_equal(np.concatenate(list(t), axis=1), panel)
    k = ALL_CHANNELS.index("depth")
    assert len(np.unique(seen[0][1][:, k * W:(k + 1) * W].reshape(-1, 3), axis=0)) > 2  # the range resolves the depths: several table entries
    # default depth range: the collider's planes
    dflt = render.render_path(model, poses[:1], H, W, *intr, ("depth", "rgb"))
    planes = render.render_path(model, poses[:1], H, W, *intr, ("depth", "rgb"), (2.0, 6.0))
    other = render.render_path(model, poses[:1], H, W, *intr, ("depth", "rgb"), depth_range)
    assert np.array_equal(dflt[0], planes[0]) and not np.array_equal(dflt[0], other[0])
    assert np.array_equal(other[0][:, :W], seen[0][1][:, k * W:(k + 1) * W])


def test_render_command_writes_panels_tiles_and_frames_json(small_model, tmp_path, capsys):
    pytest.importorskip("PIL")
    from PIL import Image

    _, model = small_model
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    run = tmp_path / "run"
    ckpt = trainer.save_checkpoint(trainer.checkpoint_path(str(run), 7), model, opt, 7)
    H, W, channels = 8, 12, ["rgb", "normals", "depth", "mask"]
    out = tmp_path / "frames"
    (out / "panel").mkdir(parents=True)
    (out / "panel" / "9999.png").write_bytes(b"kept")
    (out / "notes.txt").write_text("kept")
    (out / "frames.json").write_text("{}")
    argv = ["render", "--ckpt", str(run), "--out", str(out), "--width", str(W), "--height", str(H), "--fov-x", "40", "--radius", "4",
            "--elevation", "20", "--frames", "2", "--chunk", "64", "--channels", *channels]
    assert trainer.main(argv) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    assert "2 frames" in line and "s per frame" in line and "rays/s" in line
    # what render_path returns for the checkpoint's model (the reference sample counts: the checkpoint records only the field's shape)
    loaded, step = trainer.load_checkpoint(ckpt, None, DEV)
    loaded.config.eval_num_rays_per_chunk = 64
    poses = render.orbit_path(2, (0.0, 0.0, 0.0), 4.0, 20.0)
    intr = render.pinhole(W, H, math.radians(40.0))
    want = render.render_path(loaded, poses, H, W, *intr, channels)
    for i in range(2):
        assert np.array_equal(np.asarray(Image.open(out / "panel" / f"{i:04d}.png")), want[i])
    meta = json.loads((out / "frames.json").read_text())
    assert meta["step"] == step == 7 and meta["checkpoint"] == ckpt and meta["channels"] == channels
    assert (meta["width"], meta["height"], meta["chunk"], meta["mma"], meta["tiles"]) == (W, H, 64, "f32", False)
    assert meta["depth_range"] == [2.0, 6.0] and (meta["fx"], meta["fy"], meta["cx"], meta["cy"]) == intr
    assert [f["files"] for f in meta["frames"]] == [{"panel": "panel/0000.png"}, {"panel": "panel/0001.png"}]
    assert np.array_equal(np.float32([f["c2w"] for f in meta["frames"]]), poses)
    assert (out / "notes.txt").read_text() == "kept" and (out / "panel" / "9999.png").read_bytes() == b"kept"
    # --tiles into the same directory: one folder per channel; the panels of the first run stay
    assert trainer.main(argv + ["--tiles", "--depth-range", "1", "9"]) == 0
    want_t = render.render_path(loaded, poses, H, W, *intr, channels, (1.0, 9.0), panel=False)
    for i in range(2):
        for c, name in enumerate(channels):
            assert np.array_equal(np.asarray(Image.open(out / name / f"{i:04d}.png")), want_t[i][c])
    meta = json.loads((out / "frames.json").read_text())
    assert meta["tiles"] is True and meta["depth_range"] == [1.0, 9.0]
    assert meta["frames"][1]["files"] == {name: f"{name}/0001.png" for name in channels}
    assert sorted(os.listdir(out)) == sorted(["frames.json", "notes.txt", "panel", *channels])
    assert sorted(os.listdir(out / "panel")) == ["0000.png", "0001.png", "9999.png"]
