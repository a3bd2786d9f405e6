"""GPU checks of the TSDF mesh export: rsn_tsdf_integrate against the numpy restatement of include/rsn.h (tests/tsdf_reference.py),
bit for bit -- tiny and ragged grids, a grid past one pass of the launch, split calls, pre-filled volumes, cameras that see nothing,
projections on pixel edges, special depth values, the near plane -- its argument errors with sentinel-filled outputs, the depth-only
eval pass against the full one, and the route from a checkpoint to a PLY file on small models."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, ops, render, trainer
from reflect_sampling_nerf_amd._abi import ptr
from reflect_sampling_nerf_amd.nerfstudio_compat import RayBundle
from tests import helpers
from tests import tsdf_reference as ref
from tests.mesh_reference import OFFSETS, parse_ply

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _f3(x):
    return (C.c_float * 3)(*[float(v) for v in x])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_integrate(T0, W0, o, s, c2w, H, W, intr, depth, trunc, near):
    """One call through the public wrapper, in place on copies -> (tsdf, weight) as numpy."""
    T, Wt = torch.from_numpy(np.array(T0, dtype=np.float32)).to(DEV), torch.from_numpy(np.array(W0, dtype=np.float32)).to(DEV)
    mesh.integrate_depth(T, Wt, o, s, torch.from_numpy(np.ascontiguousarray(c2w, dtype=np.float32).reshape(-1, 3, 4)).to(DEV),
                         torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32).reshape(-1, H * W)).to(DEV), H, W, *intr,
                         trunc, near)
    torch.cuda.synchronize()
    return T.cpu().numpy(), Wt.cpu().numpy()


def assert_bits(got, want):
    for g, w, name in zip(got, want, ("tsdf", "weight")):
        bad = np.flatnonzero(bits(g).ravel() != bits(w).ravel())
        assert bad.size == 0, f"{name}: {bad.size} of {g.size} words differ, first at {bad[:5]}: {g.ravel()[bad[:5]]} != {w.ravel()[bad[:5]]}"


def check(shape_xyz, o, s, c2w, H, W, intr, depth, trunc, near, T0=None, W0=None):
    """Device == reference, bit for bit -> the reference's (tsdf, weight) and the mask of updated vertices."""
    nx, ny, nz = shape_xyz
    T0 = np.zeros((nz, ny, nx), np.float32) if T0 is None else T0
    W0 = np.zeros((nz, ny, nx), np.float32) if W0 is None else W0
    want = ref.integrate(T0, W0, o, s, c2w, H, W, *intr, depth, trunc, near)
    assert_bits(device_integrate(T0, W0, o, s, c2w, H, W, intr, depth, trunc, near), want)
    return want[0], want[1], want[1] != W0


def random_views(rng, n, centre, distance):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.stack([ref.look_at(np.asarray(centre) + distance * v, centre) for v in d])


def random_depth(rng, n, H, W, distance, spread):
    return (distance + spread * rng.uniform(-1.0, 1.0, size=(n, H * W))).astype(np.float32)


def test_one_cell_one_small_view():
    o, s = (-0.5, -0.25, -0.5), (1.0, 0.5, 1.0)
    pose = ref.look_at((0.3, -3.0, 0.2), (0.0, 0.0, 0.0))[None]
    H = W = 4
    depth = np.float32([2.6, 3.1, 3.4, 2.9] * 4).reshape(1, 16)
    _, Wt, upd = check((2, 2, 2), o, s, pose, H, W, (3.0, 3.0, 2.0, 2.0), depth, 0.75, 0.0)
    assert upd.any() and Wt.max() == 1.0


@pytest.mark.parametrize("shape_xyz", [(5, 7, 3), (33, 9, 5)])
def test_ragged_grids_three_random_views(shape_xyz):
    """No dimension is a multiple of anything; 33 x 9 x 5 = 1485 vertices span 6 workgroups, the last one partial."""
    rng = np.random.default_rng(sum(shape_xyz))
    o, s = (-1.1, -0.9, -0.4), (0.07, 0.23, 0.19)
    centre = np.float32(o) + np.float32(s) * (np.float32(shape_xyz) - 1) / 2
    H, W = 13, 17
    poses = random_views(rng, 3, centre, 3.0)
    depth = random_depth(rng, 3, H, W, 3.0, 0.6)
    _, Wt, upd = check(shape_xyz, o, s, poses, H, W, (20.0, 21.0, 8.5, 6.5), depth, 0.3, 0.0)
    assert 0 < upd.sum() < upd.size and Wt.max() == 3.0  # seen by all three, by some, hidden from or outside others


def test_a_grid_past_one_pass_of_the_launch():
    """81^3 = 531,441 vertices: more than the 2048 workgroups x 256 lanes of one pass, so the grid stride is taken."""
    n = 81
    assert n ** 3 > 2048 * 256
    rng = np.random.default_rng(81)
    h = np.float32(2.0 / (n - 1))
    poses = random_views(rng, 2, (0.0, 0.0, 0.0), 3.0)
    H, W = 13, 17
    _, _, upd = check((n, n, n), (-1.0, -1.0, -1.0), (h, h, h), poses, H, W, (22.0, 22.0, 8.5, 6.5), random_depth(rng, 2, H, W, 3.0, 0.7),
                      0.25, 0.0)
    assert upd.reshape(-1)[2048 * 256:].any() and not upd.all()


def test_five_views_equal_two_then_three_on_prefilled_volumes():
    """Views are applied in ascending order, so a call may be split anywhere; the volumes start from random T and integer W, so a
    vertex no view reaches provably keeps its bits."""
    rng = np.random.default_rng(5)
    shape_xyz, o, s = (9, 6, 7), (-0.8, -0.5, -0.6), (0.2, 0.2, 0.2)
    nx, ny, nz = shape_xyz
    T0 = rng.uniform(-1, 1, size=(nz, ny, nx)).astype(np.float32)
    W0 = rng.integers(0, 9, size=(nz, ny, nx)).astype(np.float32)
    H, W, intr = 13, 17, (40.0, 40.0, 8.5, 6.5)  # a narrow frustum: part of the grid is outside every view
    poses = random_views(rng, 5, (0.0, 0.0, 0.0), 3.0)
    depth = random_depth(rng, 5, H, W, 3.0, 0.5)
    Tw, Ww, upd = check(shape_xyz, o, s, poses, H, W, intr, depth, 0.4, 0.0, T0, W0)
    assert 0 < upd.sum() < upd.size
    assert np.array_equal(bits(Tw)[~upd], bits(T0)[~upd]) and np.array_equal(Ww[~upd], W0[~upd])
    a = device_integrate(T0, W0, o, s, poses[:2], H, W, intr, depth[:2], 0.4, 0.0)
    b = device_integrate(a[0], a[1], o, s, poses[2:], H, W, intr, depth[2:], 0.4, 0.0)
    assert_bits(b, (Tw, Ww))


def test_cameras_that_see_part_or_nothing_of_the_grid():
    rng = np.random.default_rng(7)
    shape_xyz, o, s = (8, 8, 8), (-0.7, -0.7, -0.7), (0.2, 0.2, 0.2)
    T0 = rng.uniform(-1, 1, size=(8, 8, 8)).astype(np.float32)
    W0 = rng.integers(1, 5, size=(8, 8, 8)).astype(np.float32)
    H, W, intr = 13, 17, (9.0, 9.0, 8.5, 6.5)
    # inside the grid, looking along +x: the vertices behind it, and those level with it, have z <= 0
    inside = ref.look_at((0.1, 0.05, -0.05), (5.0, 0.05, -0.05))[None]
    _, _, upd = check(shape_xyz, o, s, inside, H, W, intr, np.full((1, H * W), 0.5, np.float32), 0.4, 0.0, T0, W0)
    x = np.float32(-0.7) + np.float32(0.2) * np.arange(8, dtype=np.float32)
    assert upd.any() and not upd[:, :, x <= np.float32(0.1)].any()
    # outside, looking away from the grid: nothing is in front of it; and looking past it: in front, but outside the image
    away = ref.look_at((3.0, 0.0, 0.0), (6.0, 0.0, 0.0))[None]
    past = ref.look_at((3.0, 0.0, 0.0), (3.0, 5.0, 0.0))[None]
    for pose in (away, past):
        Tw, Ww, upd = check(shape_xyz, o, s, pose, H, W, intr, np.full((1, H * W), 3.0, np.float32), 0.4, 0.0, T0, W0)
        assert not upd.any() and np.array_equal(bits(Tw), bits(T0)) and np.array_equal(Ww, W0)


def test_projections_on_pixel_edges_and_on_the_image_border():
    """Axis-aligned pose and power-of-two numbers: every step is exact, so u and v land exactly on pixel edges.  Camera at z = 4
    looking down -z with x right and y up; grid z = 2, 0: vertex depths 2 and 4; fx = fy = 4, cx = cy = 4, 8 x 8 pixels:
    u = 4 + 4 x / z in steps of 1/2 or 1/4, u == 8 == width for x = 2 at z = 2 (outside), u == 0 for x = -2 at z = 2 (inside)."""
    c2w = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4]])[None]
    shape_xyz, o, s = (9, 9, 2), (-2.0, -2.0, 0.0), (0.5, 0.5, 2.0)
    H = W = 8
    depth = (2.0 + 0.25 * np.arange(64, dtype=np.float32)).reshape(1, 64)  # every pixel its own value: a wrong pixel shows
    Tw, Ww, upd = check(shape_xyz, o, s, c2w, H, W, (4.0, 4.0, 4.0, 4.0), depth, 16.0, 0.0)
    near_plane = upd[1]  # grid z = 2, at depth 2: u = 4 + 2 x, v = 4 - 2 y
    assert near_plane[:, 0].sum() > 0 and not near_plane[:, 8].any()  # u == 0 is inside, u == 8 == width is not
    assert not near_plane[0].any() and near_plane[8].sum() > 0        # v == 8 == height (y = -2) is not, v == 0 (y = 2) is
    # vertex (x, y, z) = (-2, 2, 2) projects onto the corner (u, v) = (0, 0): pixel 0, D = 2, r = sqrt(12)
    assert Ww[1, 8, 0] == 1.0 and Tw[1, 8, 0] == (np.float32(2.0) - np.sqrt(np.float32(12.0))) / np.float32(16.0)
    # vertex (0.5, 0, 2) projects to u = 5 exactly: the pixel to the right of the edge, x = 5, y = 4
    assert Tw[1, 4, 5] == (depth[0, 4 * 8 + 5] - np.sqrt(np.float32(4.25))) / np.float32(16.0)
    assert upd[0].all()  # z = 0 plane at depth 4: u = 4 + x in [2, 6]


def test_special_depth_values():
    rng = np.random.default_rng(11)
    shape_xyz, o, s = (7, 6, 5), (-0.6, -0.5, -0.4), (0.2, 0.2, 0.2)
    T0 = rng.uniform(-1, 1, size=(5, 6, 7)).astype(np.float32)
    W0 = rng.integers(0, 4, size=(5, 6, 7)).astype(np.float32)
    H, W = 13, 17
    poses = random_views(rng, 3, (0.0, 0.0, 0.0), 3.0)
    depth = random_depth(rng, 3, H, W, 3.0, 0.5)
    special = np.float32([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-42, 3e38])
    for n in range(3):
        depth[n, rng.choice(H * W, 15 * len(special), replace=False)] = np.repeat(special, 15)
    Tw, Ww, upd = check(shape_xyz, o, s, poses, H, W, (14.0, 14.0, 8.5, 6.5), depth, 0.4, 0.0, T0, W0)
    assert np.all(np.isfinite(Tw)) and 0 < upd.sum() < upd.size
    # maps that are special everywhere: not finite skips; negative and zero are "far behind the surface" and skip as hidden;
    # a huge finite depth carves: d = 1
    for value, touches in ((np.nan, False), (np.inf, False), (-np.inf, False), (-1.0, False), (0.0, False), (3e38, True)):
        Tw, Ww, upd = check(shape_xyz, o, s, poses[:1], H, W, (14.0, 14.0, 8.5, 6.5), np.full((1, H * W), value, np.float32), 0.4,
                            0.0, T0, W0)
        assert upd.any() == touches, value


def test_near_plane_skips_the_close_vertices():
    rng = np.random.default_rng(13)
    shape_xyz, o, s = (6, 6, 6), (-0.5, -0.5, -0.5), (0.2, 0.2, 0.2)
    H, W, intr = 13, 17, (8.0, 8.0, 8.5, 6.5)
    pose = ref.look_at((1.6, 0.2, 0.1), (0.0, 0.0, 0.0))[None]
    depth = random_depth(rng, 1, H, W, 1.6, 0.3)
    _, _, all_upd = check(shape_xyz, o, s, pose, H, W, intr, depth, 5.0, 0.0)
    _, _, upd = check(shape_xyz, o, s, pose, H, W, intr, depth, 5.0, 1.6)
    x, y, z = (np.float32(-0.5) + np.float32(0.2) * np.arange(6, dtype=np.float32) for _ in range(3))
    r = np.sqrt((x[None, None, :] - 1.6) ** 2 + (y[None, :, None] - 0.2) ** 2 + (z[:, None, None] - 0.1) ** 2)
    assert all_upd[r < 1.59].any() and not upd[r < 1.59].any() and np.array_equal(upd[r > 1.61], all_upd[r > 1.61]) and upd.any()


# ---------------------------------------------------------------------------------------------- errors and empty calls
def test_argument_errors_and_empty_calls_leave_the_volumes_alone():
    lib = _abi.load_library()
    nx, ny, nz, H, W = 5, 4, 3, 6, 7
    SENT_T, SENT_W = -12345.5, 777.0
    T = torch.full((nz, ny, nx), SENT_T, device=DEV)
    Wt = torch.full((nz, ny, nx), SENT_W, device=DEV)
    pose = torch.from_numpy(ref.look_at((0.0, -3.0, 0.0))[None]).to(DEV)
    depth = torch.full((1, H * W), 3.0, device=DEV)
    o3, s3 = _f3((-0.4, -0.3, -0.2)), _f3((0.2, 0.2, 0.2))
    nan, inf = float("nan"), float("inf")

    def call(nx=nx, ny=ny, nz=nz, o=o3, s=s3, n=1, c2w=ptr(pose), h=H, w=W, fx=9.0, fy=9.0, d=ptr(depth), trunc=0.5, near=0.0,
             t=ptr(T), wt=ptr(Wt)):
        return lib.rsn_tsdf_integrate(nx, ny, nz, o, s, n, c2w, h, w, fx, fy, 3.5, 3.0, d, trunc, near, t, wt, ops._stream())

    for kw in (dict(nx=1), dict(ny=0), dict(nz=1), dict(h=0), dict(w=-1), dict(h=2 ** 16, w=2 ** 15), dict(n=-1), dict(o=None), dict(s=None),
               dict(c2w=None), dict(d=None), dict(t=None), dict(wt=None), dict(trunc=0.0), dict(trunc=-0.5), dict(trunc=nan),
               dict(trunc=inf), dict(near=nan), dict(near=-inf), dict(fx=0.0), dict(fy=-0.0), dict(fx=inf), dict(fy=nan)):
        assert call(**kw) == INVALID, kw
        assert lib.rsn_last_error()
    assert call(nx=1024, ny=1024, nz=1024) == UNSUPPORTED
    assert call(n=0) == OK and call(n=0, c2w=None, d=None) == OK
    torch.cuda.synchronize()
    assert bool((T == SENT_T).all()) and bool((Wt == SENT_W).all())
    with pytest.raises(_abi.RsnError):
        mesh.integrate_depth(T, Wt, (0, 0, 0), (1, 1, 1), pose, depth, H, W, 9.0, 9.0, 3.5, 3.0, -1.0, 0.0)
    assert call() == OK  # and the same call with nothing wrong writes
    torch.cuda.synchronize()
    assert bool((Wt == SENT_W + 1).any())


# ---------------------------------------------------------------------------------------------- the depth-only pass
@pytest.fixture(scope="module")
def tiny_model():
    torch.manual_seed(6)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=16, num_importance_samples=16, num_reflect_coarse_samples=8,
                                            num_reflect_importance_samples=8, base_mlp_num_layers=4, base_mlp_layer_width=32,
                                            eval_num_rays_per_chunk=16)
    model = cfg.setup(scene_box=None, num_train_data=1)
    return model.to(DEV).eval()


SURFACE_KEYS = ("depth_fine", "accumulation_fine", "depth_coarse", "accumulation_coarse")


def test_surface_outputs_are_the_full_pass_bits(tiny_model):
    g = torch.Generator().manual_seed(1)
    R = 37
    o = torch.randn(R, 3, generator=g) * 0.3 + torch.tensor([0.0, -4.0, 0.0])
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g) * 0.2 + torch.tensor([0.0, 1.0, 0.0]), dim=-1)
    pa = torch.rand(R, 1, generator=g) * 1e-4 + 1e-5

    def rays():
        return RayBundle(origins=o.to(DEV), directions=d.to(DEV), pixel_area=pa.to(DEV))

    full = tiny_model(rays())
    surf = tiny_model.get_surface_outputs(rays())
    torch.cuda.synchronize()
    assert set(surf) == set(SURFACE_KEYS)
    for k in SURFACE_KEYS:
        assert surf[k].shape == (R, 1) and torch.equal(surf[k].view(torch.int32), full[k].view(torch.int32)), k
    assert float(surf["depth_fine"].min()) < float(surf["depth_fine"].max())


def test_chunked_surface_image_is_the_full_image_and_reads_nothing_back(tiny_model):
    H, W = 7, 9
    intr = render.pinhole(W, H, 0.7)
    pose = render.orbit_path(1, (0.0, 0.0, 0.0), 4.0, 20.0)[0]
    full = tiny_model.get_outputs_for_camera_ray_bundle(render.camera_rays(pose, H, W, *intr, DEV))  # 16-ray chunks: 3 full, one of 15
    rays = render.camera_rays(pose, H, W, *intr, DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        surf = tiny_model.get_surface_outputs_for_camera_ray_bundle(rays, 16)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in SURFACE_KEYS:
        assert surf[k].shape == (H, W, 1) and torch.equal(surf[k].view(torch.int32), full[k].view(torch.int32)), k
    other = tiny_model.get_surface_outputs_for_camera_ray_bundle(rays, 1000)  # one chunk, and the config's default
    assert torch.equal(other["depth_fine"], surf["depth_fine"])
    assert torch.equal(tiny_model.get_surface_outputs_for_camera_ray_bundle(rays)["depth_fine"], surf["depth_fine"])


# ---------------------------------------------------------------------------------------------- checkpoint -> PLY
RES, BOUNDS, SIDE, FOV_DEG = 12, (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), 16, 40.0
FOG_DEPTH = helpers.FOG_DEPTH


@pytest.fixture(scope="module")
def fog_checkpoint(tmp_path_factory):
    """A 4 x 64 field whose density head is a constant: a fog of sigma = ln 2 / 3.5, so every eval ray (near plane 0) has its
    median depth about 3.5 from its camera, wherever it looks.  From cameras 4 away from the origin the fused surface is then the
    part of the spheres of radius 3.5 around the cameras that lies in the box: zero crossings between observed vertices."""
    return helpers.fog_checkpoint(tmp_path_factory.mktemp("fog") / "run", DEV)


def orbit_cameras():
    fx, fy, cx, cy = render.pinhole(SIDE, SIDE, math.radians(FOV_DEG))
    return {"c2w": render.orbit_path(4, (0.0, 0.0, 0.0), 4.0, 20.0), "width": SIDE, "height": SIDE, "fx": fx, "fy": fy, "cx": cx, "cy": cy}


def test_export_mesh_tsdf_end_to_end(fog_checkpoint, tmp_path, capsys):
    ckpt, run = fog_checkpoint
    cams = orbit_cameras()
    res = mesh.export_mesh(ckpt, str(tmp_path / "a.ply"), resolution=RES, bounds=BOUNDS, method="tsdf", cameras=cams)
    h = 3.0 / (RES - 1)
    assert (res["method"], res["views"], res["min_weight"], res["step"]) == ("tsdf", 4, 1.0, 5) and "iso" not in res
    assert res["trunc"] == 4.0 * float(np.float32(h)) and res["image"] == [SIDE, SIDE]
    assert set(res["seconds"]) == {"depth", "integrate", "count", "emit", "filter", "attributes", "write"}
    assert all(t >= 0 for t in res["seconds"].values())
    assert 0 < res["triangles"] <= res["triangles_extracted"] and 0 < res["vertices"] <= res["vertices_extracted"]
    # the same through the command line: transforms-format poses with the size and the field of view
    frames = [{"file_path": f"./{i}", "transform_matrix": np.vstack([m, [[0, 0, 0, 1]]]).tolist()} for i, m in enumerate(cams["c2w"].astype(np.float64))]
    poses = tmp_path / "poses.json"
    poses.write_text(json.dumps({"camera_angle_x": math.radians(FOV_DEG), "w": SIDE, "h": SIDE, "frames": frames}))
    argv = ["export-mesh", "--method", "tsdf", "--ckpt", run, "--out", str(tmp_path / "b.ply"), "--resolution", str(RES), "--poses", str(poses)]
    assert trainer.main(argv) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    assert f"{res['vertices']} vertices, {res['triangles']} triangles" in line and "4 depth maps 16 x 16" in line
    blob = open(tmp_path / "a.ply", "rb").read()
    assert open(tmp_path / "b.ply", "rb").read() == blob  # two runs, one of them through the parser: identical bytes
    vert, faces, _ = parse_ply(str(tmp_path / "a.ply"))
    assert len(vert["x"]) == res["vertices"] and faces.shape == (res["triangles"], 3)
    assert faces.min() == 0 and faces.max() == res["vertices"] - 1 and len(np.unique(faces)) == res["vertices"]
    # the stages by hand on the checkpoint's model: the file's vertices are the kept ones, each on an edge between observed vertices
    model, _ = trainer.load_checkpoint(ckpt, None, DEV)
    model.field.set_mma_mode("f32")
    (nx, ny, nz), origin, spacing = mesh.grid_frame(BOUNDS, RES)
    intr = (cams["fx"], cams["fy"], cams["cx"], cams["cy"])
    tsdf, weight = mesh.fuse_depth(model, cams["c2w"], SIDE, SIDE, *intr, BOUNDS, RES, res["trunc"])
    split = mesh.fuse_depth(model, cams["c2w"], SIDE, SIDE, *intr, BOUNDS, RES, res["trunc"], views_per_launch=3, chunk=100)
    assert torch.equal(split[0].view(torch.int32), tsdf.view(torch.int32)) and torch.equal(split[1], weight)
    full = mesh.extract_surface(mesh.tsdf_volume(tsdf, weight, 1.0), 0.0, origin, spacing)
    kept = mesh.drop_unobserved(full, weight, (nx, ny, nz), 1.0)
    assert (full["positions"].shape[0], full["triangles"].shape[0]) == (res["vertices_extracted"], res["triangles_extracted"])
    pos = np.stack([vert["x"], vert["y"], vert["z"]], 1)
    assert np.array_equal(pos, kept["positions"].cpu().numpy()) and np.array_equal(faces, kept["triangles"].cpu().numpy())
    w = weight.cpu().numpy()
    key = kept["vert_key"].cpu().numpy().astype(np.int64)
    lo_pt = np.float32(origin)
    for p, k in zip(pos, key):
        v, d = divmod(int(k), 8)
        ijk = np.array([v % nx, (v // nx) % ny, v // (nx * ny)])
        far = ijk + np.array(OFFSETS[d])
        assert w[ijk[2], ijk[1], ijk[0]] >= 1.0 and w[far[2], far[1], far[0]] >= 1.0
        a, b = lo_pt + np.float32(spacing) * ijk.astype(np.float32), lo_pt + np.float32(spacing) * far.astype(np.float32)
        assert np.all(p >= np.minimum(a, b)) and np.all(p <= np.maximum(a, b))  # inside the edge's box, and on its line:
        t = (p - a)[OFFSETS[d].index(1)] / (b - a)[OFFSETS[d].index(1)]
        assert np.allclose(p, a + t * (b - a), atol=1e-6)
    # the fog's surface: about FOG_DEPTH from the nearest camera that sees the vertex -- within a truncation of it
    dist = np.linalg.norm(pos[:, None, :] - cams["c2w"][None, :, :, 3], axis=2)
    assert np.all(np.abs(dist - FOG_DEPTH).min(axis=1) < res["trunc"])
    nrm = np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-5)


def test_density_route_writes_what_its_stages_write(tmp_path):
    """The existing route, composed by hand from the public stages as before this method switch existed, against export_mesh with
    and without the new keyword: the same bytes."""
    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)
    model = trainer.make_model(cfg, seed=3).to(DEV).eval()
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ckpt = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "run"), 7), model, opt, 7)
    res, bounds = 20, (-1.2, -1.2, -1.2, 1.2, 1.2, 1.2)
    iso = float(mesh.density_grid(model.field, bounds, res, mma="f32").median())
    a = mesh.export_mesh(ckpt, str(tmp_path / "a.ply"), resolution=res, bounds=bounds, iso=iso)
    b = mesh.export_mesh(ckpt, str(tmp_path / "b.ply"), resolution=res, bounds=bounds, iso=iso, method="density")
    assert a["method"] == b["method"] == "density" and a["iso"] == iso and a["triangles"] > 0
    assert set(a["seconds"]) == {"grid", "count", "emit", "attributes", "write"}
    loaded, _ = trainer.load_checkpoint(ckpt, None, DEV)
    loaded.field.set_mma_mode("f32")
    _, origin, spacing = mesh.grid_frame(bounds, res)
    m = mesh.extract_surface(mesh.density_grid(loaded.field, bounds, res), iso, origin, spacing)
    m.update(mesh.vertex_attributes(loaded.field, m["positions"], spacing))
    mesh.write_ply(str(tmp_path / "c.ply"), m)
    want = open(tmp_path / "c.ply", "rb").read()
    assert open(tmp_path / "a.ply", "rb").read() == want and open(tmp_path / "b.ply", "rb").read() == want
    with pytest.raises(ValueError):
        mesh.export_mesh(ckpt, str(tmp_path / "d.ply"), method="tsdf")  # no cameras
