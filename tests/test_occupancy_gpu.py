"""GPU checks of empty-space skipping: rsn_occupancy_build bit for bit against the rule, rsn_occupancy_cull between the two
predicates of tests/occupancy_reference.py, rsn_scatter_rows, the model's culled eval path against its own unculled one (hit rays:
the same bits; culled rays: the documented values; no host read), the quality on the trained fixture, and the two commands."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, occupancy, ops, render, trainer
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import occupancy_reference as ref
from tests.helpers import load_golden

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 0x5A5A5A5A
POISON = -7.25e11


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _c3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# ------------------------------------------------------------------------------------------------ build
def device_build(vol, threshold, dilate):
    """-> (the words of the bit array, the guard words in front of and behind it)."""
    lib = _abi.load_library()
    nz, ny, nx = vol.shape
    nbytes = int(lib.rsn_occupancy_bytes(nx, ny, nz))
    assert nbytes == 4 * ref.n_words((nx, ny, nz))
    buf = torch.full((nbytes // 4 + 4,), GUARD, device=DEV, dtype=torch.int32)
    bits = buf[2:2 + nbytes // 4]
    vol_dev = _dev(vol)  # held until the launch has run: a temporary's memory would go back to the allocator at once
    check(lib.rsn_occupancy_build(nx, ny, nz, ptr(vol_dev), float(threshold), dilate, ptr(bits), nbytes, ops._stream()))
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    return host[2:-2], np.concatenate([host[:2], host[-2:]])


@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("dims", ref.DIMS, ids=lambda d: "x".join(map(str, d)))
def test_build_is_the_rule_bit_for_bit(dims, dilate):
    threshold = 0.5
    vol = ref.build_volume(dims, 7 * dilate + dims[0], threshold)
    assert np.isnan(vol).any() and np.isposinf(vol).any() and np.isneginf(vol).any() and (vol == np.float32(threshold)).any()
    want = ref.pack_bits(ref.build_cells(vol, threshold, dilate))
    got, guards = device_build(vol, threshold, dilate)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert np.all(guards == GUARD)
    cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    if cells % 32:
        assert int(got[-1]) >> (cells % 32) == 0  # the pad bits
    again, _ = device_build(vol, threshold, dilate)
    assert np.array_equal(again, got)
    for fill, full in ((0.0, False), (1.0, True), (np.nan, True)):
        flat = np.full(vol.shape, fill, dtype=np.float32)
        got, guards = device_build(flat, threshold, dilate)
        assert np.array_equal(got, ref.pack_bits(np.full(tuple(n - 1 for n in vol.shape), full))) and np.all(guards == GUARD)


def test_build_and_size_argument_errors():
    lib = _abi.load_library()
    assert lib.rsn_occupancy_bytes(1, 4, 4) == 0 and b"dimension" in lib.rsn_last_error()
    assert lib.rsn_occupancy_bytes(1024, 1024, 129) == 0
    assert lib.rsn_occupancy_bytes(512, 512, 512) == 4 * ((511 ** 3 + 31) // 32)
    vol, bits = torch.zeros(27, device=DEV), torch.zeros(1, device=DEV, dtype=torch.int32)
    assert lib.rsn_occupancy_build(3, 3, 3, ptr(vol), 0.5, 3, ptr(bits), 4, None) == -1 and b"dilate" in lib.rsn_last_error()
    assert lib.rsn_occupancy_build(3, 3, 3, ptr(vol), 0.5, 1, ptr(bits), 3, None) == -1 and b"bytes" in lib.rsn_last_error()
    assert lib.rsn_occupancy_build(3, 3, 3, None, 0.5, 1, ptr(bits), 4, None) == -1
    assert lib.rsn_scatter_rows(4, None, None, None, 1, 0.0, None, None) == -1
    assert lib.rsn_scatter_rows(4, None, ptr(bits), ptr(vol), 0, 0.0, ptr(vol), None) == -1
    assert lib.rsn_occupancy_cull(-1, None, None, None, None, 3, 3, 3, _c3((0, 0, 0)), _c3((1, 1, 1)), None, 1, None, None, None, None, None) == -1
    assert lib.rsn_occupancy_cull(4, None, None, None, None, 3, 3, 3, _c3((0, 0, 0)), _c3((1, 0, 1)), None, 1, None, ptr(bits), None, None, None) == -1
    assert b"spacing" in lib.rsn_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ cull
def device_cull(dims, origin, spacing, bits, outside, o, d, near, far):
    lib = _abi.load_library()
    n = len(near)
    hit = torch.full((n + 8,), 0xA5, device=DEV, dtype=torch.uint8)
    idx = torch.full((n + 8,), -5, device=DEV, dtype=torch.int32)
    n_hit = torch.full((3,), -5, device=DEV, dtype=torch.int32)
    ws = torch.empty(max(1, int(lib.rsn_occupancy_cull_workspace_bytes(n)) // 4), device=DEV, dtype=torch.int32)
    args = [_dev(a) for a in (o, d, near, far)] if n else [None] * 4
    check(lib.rsn_occupancy_cull(n, *[ptr(a) for a in args], *dims, _c3(origin), _c3(spacing), ptr(bits), int(outside), ptr(hit[4:]),
                                 ptr(n_hit[1:]), ptr(idx[4:]), ptr(ws), ops._stream()))
    torch.cuda.synchronize()
    hit, idx, n_hit = hit.cpu().numpy(), idx.cpu().numpy(), n_hit.cpu().numpy()
    assert np.all(hit[:4] == 0xA5) and np.all(hit[4 + n:] == 0xA5) and np.all(idx[:4] == -5) and np.all(idx[4 + n:] == -5)
    assert n_hit[0] == -5 and n_hit[2] == -5
    return hit[4:4 + n], int(n_hit[1]), idx[4:4 + n]


@pytest.mark.parametrize("outside", [False, True], ids=["inside_only", "outside_occupied"])
@pytest.mark.parametrize("share", [0.05, 0.5])
@pytest.mark.parametrize("gi", range(len(ref.DIMS)), ids=["x".join(map(str, d)) for d in ref.DIMS])
def test_cull_lies_between_the_two_predicates(gi, share, outside):
    dims = ref.DIMS[gi]
    si = (0.05, 0.5).index(share)
    origin, spacing = ref.grid_frame(dims, gi)
    occ = ref.grid_case(dims, share, 2 * gi + si)
    bits = _dev(ref.pack_bits(occ).view(np.int32), np.int32)
    none3, none1 = np.zeros((0, 3), np.float32), np.zeros(0, np.float32)
    hit, n_hit, idx = device_cull(dims, origin, spacing, bits, outside, none3, none3, none1, none1)
    assert n_hit == 0 and len(hit) == 0
    for n in ref.RAY_COUNTS:
        o, d, near, far, fam = ref.ray_cases(dims, origin, spacing, n, 100 * gi + 10 * si + n)
        hit, n_hit, idx = device_cull(dims, origin, spacing, bits, outside, o, d, near, far)
        assert set(np.unique(hit)) <= {0, 1}
        must = ref.hits_shrunk(o, d, near, far, occ, origin, spacing, outside)
        may = ref.hits_grown(o, d, near, far, occ, origin, spacing, outside)
        culled_wrongly, flagged_wrongly = np.flatnonzero(must & (hit == 0)), np.flatnonzero(~may & (hit == 1))
        assert len(culled_wrongly) == 0, (n, culled_wrongly[:5], fam[culled_wrongly[:5]])
        assert len(flagged_wrongly) == 0, (n, flagged_wrongly[:5], fam[flagged_wrongly[:5]])
        assert hit[ref.invalid_rays(o, d, near, far)].all()
        assert n_hit == int(hit.sum())
        assert np.array_equal(idx, ref.expected_index(hit))
        hit2, n_hit2, idx2 = device_cull(dims, origin, spacing, bits, outside, o, d, near, far)
        assert np.array_equal(hit2, hit) and n_hit2 == n_hit and np.array_equal(idx2, idx)
        if n == 1025:
            print(f"{dims} share {share} outside {outside}: {n_hit} of {n} flagged, {int((must != may).sum())} undecided")


def test_rays_in_face_planes_are_decided_the_same_way_twice():
    for gi, dims in enumerate(ref.DIMS):
        origin, spacing = ref.grid_frame(dims, gi)
        occ = ref.grid_case(dims, 0.5, 2 * gi + 1)
        bits = _dev(ref.pack_bits(occ).view(np.int32), np.int32)
        rays = ref.face_plane_rays(dims, origin, spacing, 257, gi)
        for outside in (False, True):
            hit, n_hit, idx = device_cull(dims, origin, spacing, bits, outside, *rays)
            hit2, n_hit2, idx2 = device_cull(dims, origin, spacing, bits, outside, *rays)
            assert np.array_equal(hit, hit2) and n_hit == n_hit2 == int(hit.sum()) and np.array_equal(idx, idx2)
            assert np.array_equal(idx, ref.expected_index(hit)) and set(np.unique(hit)) <= {0, 1}


# ------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("row", [1, 3, 48])
def test_scatter_rows(row):
    lib = _abi.load_library()
    rng = np.random.default_rng(row)
    R = 777
    perm = rng.permutation(R).astype(np.int32)
    src = rng.normal(size=(R, row)).astype(np.float32)
    perm_dev = _dev(perm, np.int32)
    for count in (0, 1, 300, R - 1, R, None, R + 5):
        live = R if count is None else min(count, R)
        s = src.copy()
        s[live:] = POISON
        out = torch.full((R + 2, row), 3.5, device=DEV)
        n_dev = None if count is None else torch.tensor([count], device=DEV, dtype=torch.int32)
        s_dev = _dev(s)  # held, like perm_dev, until the launch has run
        check(lib.rsn_scatter_rows(R, ptr(n_dev), ptr(perm_dev), ptr(s_dev), row, float("nan"), ptr(out[1:]), ops._stream()))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.all(got[0] == 3.5) and np.all(got[-1] == 3.5)
        want = np.full((R, row), np.nan, dtype=np.float32)
        want[perm[:live]] = src[:live]
        assert np.array_equal(got[1:-1].view(np.int32), want.view(np.int32))
        assert not np.any(got == np.float32(POISON))
    # through the wrapper, with a trailing shape
    x = torch.randn(R, 4, 3, device=DEV)
    full = occupancy.scatter_rows(x, perm_dev, None, 0.0)
    assert torch.equal(full[perm_dev.long()], x)
    # an index outside 0 .. n_rows - 1 is skipped, not written through
    wild = perm_dev.clone()
    wild[5], wild[6] = -1, R
    out = torch.full((R + 2, row), 3.5, device=DEV)
    src_dev = _dev(src)
    check(lib.rsn_scatter_rows(R, None, ptr(wild), ptr(src_dev), row, 0.0, ptr(out[1:]), ops._stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[0] == 3.5) and np.all(got[-1] == 3.5) and np.all(got[1 + perm[5]] == 3.5) and np.all(got[1 + perm[6]] == 3.5)
    keep = np.ones(R, dtype=bool)
    keep[[5, 6]] = False
    assert np.array_equal(got[1:-1][perm[keep]], src[keep])
    assert lib.rsn_scatter_rows(0, None, None, None, row, 0.0, None, ops._stream()) == 0


# ------------------------------------------------------------------------------------------------ model
H, W = 10, 33
INTR = render.pinhole(W, H, 0.7)
POSES = render.orbit_path(2, (0.0, 0.0, 0.0), 4.0, 20.0)
ONE_KEYS = ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine", "diff")
FAR_KEYS = ("depth_coarse", "depth_fine")


def make_model(layers, width, seed=4):
    """The model of test_render_path_gpu.small_model, built afresh (4 x 64) or at 8 x 256: 16 / 16 / 8 / 8 samples, chunk 64.  Its
    collider keeps the near plane in eval mode (2 .. 6), so that the segments of cameras at radius 4 lie inside the grid's box."""
    torch.manual_seed(seed)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=16, num_importance_samples=16, num_reflect_coarse_samples=8,
                                            num_reflect_importance_samples=8, base_mlp_num_layers=layers, base_mlp_layer_width=width,
                                            eval_num_rays_per_chunk=64)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 1.5
    model.collider.reset_near_plane = False
    return model.to(DEV).eval()


def ball_grid():
    """Not from the field: a ball of radius 0.6 in [-3, 3]^3 at 33^3 vertices, outside counted as occupied."""
    n = 33
    ax = np.linspace(-3.0, 3.0, n)
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (x * x + y * y + z * z <= 0.36).astype(np.float32)
    _, origin, spacing = pkg.mesh.grid_frame((-3, -3, -3, 3, 3, 3), n)
    return occupancy.occupancy_from_volume(_dev(vol), origin, spacing, 0.5, 1, True)


def rows_equal(a, b):
    """[n, ...] tensors -> bool [n]: the rows hold the same bits."""
    n = a.shape[0]
    if a.dtype != torch.bool:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return (a.reshape(n, -1) == b.reshape(n, -1)).all(dim=1)


def same_bits(a, b):
    return a.shape == b.shape and bool(rows_equal(a.reshape(1, -1), b.reshape(1, -1)).all())


def check_culled_against_plain(model, grid, label):
    """One image with and without the grid; -> (hit [n] bool, plain outputs, culled outputs)."""
    n = H * W
    rays = render.camera_rays(POSES[0], H, W, *INTR, DEV)
    model.occupancy = None
    plain = model.get_outputs_for_camera_ray_bundle(rays)
    model.occupancy = grid
    model.get_outputs_for_camera_ray_bundle(rays)  # warm-up: streams and packed weights exist
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        culled = model.get_outputs_for_camera_ray_bundle(rays)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    flat = model.collider(rays.get_row_major_sliced_ray_bundle(0, n))
    c = occupancy.cull(grid, flat.origins.contiguous(), flat.directions.contiguous(), flat.nears.reshape(n).contiguous(),
                       flat.fars.reshape(n).contiguous())
    hit = c["hit"].bool()
    n_hit = int(c["n_hit"])
    print(f"{label}: {n - n_hit} of {n} rays culled")
    assert 0 < n - n_hit < n and int(hit.sum()) == n_hit
    assert set(culled) == set(plain) and "depth_reflect_fine" not in culled
    for k in plain:
        a, b = plain[k].reshape(n, -1), culled[k].reshape(n, -1)
        assert culled[k].shape == plain[k].shape and culled[k].dtype == plain[k].dtype, k
        bad = torch.nonzero(hit & ~rows_equal(a, b))[:, 0].tolist()
        assert not bad, f"{label} {k}: {len(bad)} hit rays differ from the unculled render, e.g. rays {bad[:5]}"
        gone = b[~hit]
        if k in ONE_KEYS:
            assert bool((gone == 1.0).all()), k
        elif k in FAR_KEYS:
            assert bool((gone == flat.fars.reshape(n, 1)[~hit]).all()) and bool((gone == 6.0).all()), k
        elif k == "mask":
            assert not bool(gone.any())
        else:
            assert bool((gone == 0.0).all()), k
    print(f"{label}: {int(plain['mask'].sum())} rays reflected, {int((plain['mask'].reshape(n) & hit).sum())} of them hit")
    return hit, plain, culled


def test_small_model_culled_image_hit_rays_keep_their_bits():
    model = make_model(4, 64)
    fresh = model.get_outputs_for_camera_ray_bundle(render.camera_rays(POSES[0], H, W, *INTR, DEV))  # before the attribute is touched
    grid = ball_grid()
    assert 0.0 < grid.occupied_share() < 0.1
    hit, plain, culled = check_culled_against_plain(model, grid, "4 x 64 f32")
    assert all(same_bits(fresh[k], plain[k]) for k in fresh) and set(fresh) == set(plain)
    del model.occupancy  # a model that never had it
    assert getattr(model, "occupancy", None) is None
    bare = model.get_outputs_for_camera_ray_bundle(render.camera_rays(POSES[0], H, W, *INTR, DEV))
    assert all(same_bits(fresh[k], bare[k]) for k in fresh)
    # get_outputs on a flat bundle: the same rows, and the lazy [M, 1] entry lists the reflected rays as before
    model.occupancy = grid
    n = H * W
    flat = model.collider(render.camera_rays(POSES[0], H, W, *INTR, DEV).get_row_major_sliced_ray_bundle(0, n))
    torch.cuda.set_sync_debug_mode("error")
    try:
        one = model(flat)
        present = dict(one.present())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k, v in present.items():
        assert same_bits(v.reshape(n, -1), culled[k].reshape(n, -1)), k
    model.occupancy = None
    ref_one = model(flat)
    # ... of the rays that are rendered: a culled ray is never reflected, so its row of the unculled list is absent
    reflected = plain["mask"].reshape(n)
    if int((reflected & hit).sum()):
        want = ref_one["depth_reflect_fine"][hit[reflected]]
        assert one["depth_reflect_fine"].shape == want.shape == (int((reflected & hit).sum()), 1)
        assert same_bits(one["depth_reflect_fine"], want)
    else:
        assert "depth_reflect_fine" not in one
    assert grid.rays_seen >= 3 * n and 0.0 < grid.culled_share() < 1.0
    # training never uses the grid
    model.occupancy = grid
    model.train()
    seen = grid.rays_seen
    model(flat[:32])
    assert grid.rays_seen == seen
    model.eval()


@pytest.mark.parametrize("mma", ["f32", "bf16x6", "bf16"])
def test_full_width_model_culled_image_hit_rays_keep_their_bits(mma):
    model = make_model(8, 256, seed=5)
    model.field.set_mma_mode(mma)
    check_culled_against_plain(model, ball_grid(), f"8 x 256 {mma}")


def test_render_path_with_a_grid_issues_no_host_read():
    model = make_model(4, 64)
    channels = tuple(render.CHANNELS)
    plain = render.render_path(model, POSES, H, W, *INTR, channels)
    model.occupancy = ball_grid()
    render.render_path(model, POSES[:1], H, W, *INTR, channels)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        culled = render.render_path(model, POSES, H, W, *INTR, channels)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    n = H * W
    for i in range(2):
        flat = model.collider(render.camera_rays(POSES[i], H, W, *INTR, DEV).get_row_major_sliced_ray_bundle(0, n))
        c = occupancy.cull(model.occupancy, flat.origins.contiguous(), flat.directions.contiguous(), flat.nears.reshape(n).contiguous(),
                           flat.fars.reshape(n).contiguous())
        hit = c["hit"].bool().view(H, W).cpu().numpy()
        assert 0 < hit.sum() < n
        a, b = plain[i].reshape(H, len(channels), W, 3), culled[i].reshape(H, len(channels), W, 3)
        for ci, name in enumerate(channels):
            assert np.array_equal(a[:, ci][hit], b[:, ci][hit]), name
        rgb = b[:, channels.index("rgb")]
        assert np.all(rgb[~hit] == 255)  # a culled pixel is the white background


# ------------------------------------------------------------------------------------------------ quality on the trained fixture
def trained_model():
    meta, g = load_golden("eval_trained_l8_w256")
    s = meta["samples"]
    assert list(s) == [32, 32, 16, 16] and (meta["layers"], meta["width"]) == (8, 256)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=s[0], num_importance_samples=s[1], num_reflect_coarse_samples=s[2],
                                            num_reflect_importance_samples=s[3], base_mlp_num_layers=8, base_mlp_layer_width=256)
    model = cfg.setup(scene_box=None, num_train_data=1)
    model.field.load_state_dict(g["param"], strict=True)
    return model.to(DEV).eval()


def test_quality_on_the_trained_fixture():
    """The 40 x 40 view of the CPU experiment (radius 4, azimuth 30, elevation 25 degrees, horizontal field of view 50 degrees, near
    2, far 6) with the 96^3 grid over [-3, 3]^3 at the defaults: at least 30 % of the rays are culled (the experiment: 45 % with a
    traversal that culls a superset), and no colour of a culled ray moves by more than 0.03 (the experiment: 0.0205)."""
    model = trained_model()
    S = 40
    rays = render.camera_rays(render.orbit_path(1, (0.0, 0.0, 0.0), 4.0, 25.0, 30.0)[0], S, S, *render.pinhole(S, S, np.radians(50.0)), DEV)
    rays.nears = torch.full((S, S, 1), 2.0, device=DEV)
    rays.fars = torch.full((S, S, 1), 6.0, device=DEV)
    plain = model.get_outputs_for_camera_ray_bundle(rays)
    grid = occupancy.build_occupancy(model.field, (-3.0, -3.0, -3.0, 3.0, 3.0, 3.0), 96)
    assert (grid.threshold, grid.dilate, grid.outside_occupied) == (0.01, 1, True)
    model.occupancy = grid
    culled = model.get_outputs_for_camera_ray_bundle(rays)
    share = grid.culled_share()
    flat = rays.get_row_major_sliced_ray_bundle(0, S * S)
    gone = occupancy.cull(grid, flat.origins.contiguous(), flat.directions.contiguous(), flat.nears.reshape(-1).contiguous(),
                          flat.fars.reshape(-1).contiguous())["hit"] == 0
    assert bool((culled["accumulation_fine"].reshape(-1)[gone] == 0.0).all()) and bool((culled["depth_fine"].reshape(-1)[gone] == 6.0).all())
    worst, where = 0.0, None
    for k in ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine"):
        diff = (culled[k] - plain[k]).abs().reshape(S * S, 3).amax(dim=1) * gone
        if float(diff.max()) > worst:
            worst, where = float(diff.max()), (k, int(diff.argmax()))
    print(f"occupied cells {grid.occupied_share():.3f}, culled share {share:.4f} ({int(gone.sum())} rays), largest colour change {worst:.5f} at {where}")
    assert abs(float(gone.float().mean()) - share) < 1e-6
    assert share >= 0.30
    assert worst <= 0.03, f"{worst} at {where}; accumulation_fine there {float(plain['accumulation_fine'].reshape(-1)[where[1]])}"


# ------------------------------------------------------------------------------------------------ commands
def test_render_and_eval_commands_with_and_without_skip_empty(tmp_path):
    pytest.importorskip("PIL")
    from PIL import Image

    model = trained_model()
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ckpt = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "run"), 3), model, opt, 3)
    Hc, Wc = 12, 16
    base = ["render", "--ckpt", ckpt, "--width", str(Wc), "--height", str(Hc), "--fov-x", "50", "--radius", "4", "--elevation", "25",
            "--frames", "2", "--chunk", "64", "--channels", "rgb", "accumulation"]
    outs = {}
    for name, extra in (("a", []), ("b", []), ("skip", ["--skip-empty", "--occupancy-resolution", "64"])):
        outs[name] = tmp_path / name
        assert trainer.main(base + ["--out", str(outs[name])] + extra) == 0
    metas = {k: json.loads((v / "frames.json").read_text()) for k, v in outs.items()}
    assert "occupancy" not in metas["a"] and set(metas["a"]) == set(metas["b"]) and set(metas["skip"]) == set(metas["a"]) | {"occupancy"}
    for i in range(2):
        assert (outs["a"] / "panel" / f"{i:04d}.png").read_bytes() == (outs["b"] / "panel" / f"{i:04d}.png").read_bytes()
    occ = metas["skip"]["occupancy"]
    print("render --skip-empty:", occ)
    assert occ["resolution"] == [64, 64, 64] and occ["sigma"] == 0.01 and occ["dilate"] == 1 and len(occ["bounds"]) == 6
    assert 0.0 < occ["occupied_share"] < 1.0 and 0.0 < occ["culled_share"] < 1.0 and occ["rays"] == 2 * Hc * Wc
    white = np.asarray(Image.open(outs["skip"] / "panel" / "0000.png"))[:, :Wc]
    assert (white == 255).all(axis=-1).mean() >= occ["culled_share"] / 2  # culled pixels are white
    # eval on a two-view scene
    scene = tmp_path / "scene"
    (scene / "test").mkdir(parents=True)
    rng = np.random.default_rng(0)
    frames = []
    for k, pose in enumerate(render.orbit_path(2, (0.0, 0.0, 0.0), 4.0, 25.0, 30.0)):
        Image.fromarray(rng.integers(0, 256, size=(Hc, Wc, 4), dtype=np.uint8), "RGBA").save(scene / "test" / f"r_{k}.png")
        frames.append({"file_path": f"./test/r_{k}", "transform_matrix": np.vstack([pose, [0, 0, 0, 1]]).tolist()})
    (scene / "transforms_test.json").write_text(json.dumps({"camera_angle_x": float(np.radians(50.0)), "frames": frames}))
    ev = ["eval", "--data", str(scene), "--ckpt", ckpt]
    assert trainer.main(ev + ["--out", str(tmp_path / "m0.json")]) == 0
    assert trainer.main(ev + ["--out", str(tmp_path / "m1.json"), "--skip-empty", "--occupancy-resolution", "64"]) == 0
    m0, m1 = json.loads((tmp_path / "m0.json").read_text()), json.loads((tmp_path / "m1.json").read_text())
    assert "occupancy" not in m0 and set(m1) == set(m0) | {"occupancy"}
    print("eval --skip-empty:", m1["occupancy"])
    assert 0.0 < m1["occupancy"]["culled_share"] < 1.0 and m1["occupancy"]["rays"] == 2 * Hc * Wc
