"""GPU checks of the point-cloud export: rsn_pointcloud_mark / rsn_pointcloud_select against the numpy restatement of include/rsn.h
(tests/pointcloud_reference.py), bit for bit and on the rays render.camera_rays returns for the same cameras -- every clause of the
candidate rule on a 5 x 3 image, ragged sizes, calls longer than one pass of the workgroups, thinning collisions, split calls on a
shared owner, empty inputs -- and the route from a checkpoint to a PLY file on a small model."""
import json
import math

import numpy as np
import pytest
import torch

from reflect_sampling_nerf_amd import _abi, pointcloud, render, trainer
from tests import helpers
from tests import pointcloud_reference as ref
from tests import tsdf_reference as tref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT_I, SENT_F = -77, -12345.5
NAN, INF = float("nan"), float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_rays(poses, H, W, intr):
    """The rays of render.camera_rays for every pose -> (origins, directions) fp32 numpy [n, H*W, 3]."""
    o, d = [], []
    for m in poses:
        r = render.camera_rays(np.asarray(m, dtype=np.float32), H, W, *intr, DEV)
        o.append(r.origins.reshape(H * W, 3).cpu().numpy())
        d.append(r.directions.reshape(H * W, 3).cpu().numpy())
    return np.stack(o), np.stack(d)


def device_pair(owner, poses, H, W, intr, depth, acc, view0, dims, o3, s3, min_acc, edge, run_mark=True):
    """One mark + select pair through the public wrappers on sentinel-filled outputs -> (owner after, n_points, pixel_index [all
    rows], positions [all rows], candidate count) as numpy."""
    n = len(poses)
    t_pose = torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 3, 4)).to(DEV)
    t_depth = torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32).reshape(n, H * W)).to(DEV)
    t_acc = None if acc is None else torch.from_numpy(np.ascontiguousarray(acc, dtype=np.float32).reshape(n, H * W)).to(DEV)
    t_owner = None if owner is None else torch.from_numpy(np.array(owner, dtype=np.int32)).to(DEV)
    views = (dims, o3, s3, t_pose, t_depth, t_acc, H, W, *intr, view0, min_acc, edge)
    if run_mark:
        pointcloud.mark(t_owner, *views)
    rows = n * H * W
    nbytes = int(_abi.load_library().rsn_pointcloud_workspace_bytes(n, H, W))
    out = (torch.full((2,), SENT_I, device=DEV, dtype=torch.int32), torch.full((rows,), SENT_I, device=DEV, dtype=torch.int32),
           torch.full((rows, 3), SENT_F, device=DEV, dtype=torch.float32), torch.empty(nbytes, device=DEV, dtype=torch.uint8))
    counts, index, pos = pointcloud.select(t_owner, *views, out=out)
    torch.cuda.synchronize()
    kept, cand = counts.tolist()
    return None if owner is None else t_owner.cpu().numpy(), kept, index.cpu().numpy(), pos.cpu().numpy(), cand


def check(owner, poses, H, W, intr, depth, acc, view0, dims, o3, s3, min_acc, edge):
    """Device == reference, bit for bit, and the rows past the count untouched -> the reference's (owner, n, index, positions,
    candidate mask, cells)."""
    ro, rd = device_rays(poses, H, W, intr)
    want = ref.mark_select(owner, ro, rd, depth, acc, H, W, view0, dims, o3, s3, min_acc, edge)
    got = device_pair(owner, poses, H, W, intr, depth, acc, view0, dims, o3, s3, min_acc, edge)
    w_owner, n, w_index, w_pos = want[:4]
    print(f"{len(poses)} views {W} x {H}, grid {dims}: {want[4].sum()} candidates, {n} kept")
    assert got[1] == n and got[4] == want[4].sum()  # kept rows, and the candidates before the owner test
    assert np.array_equal(got[2][:n], w_index) and np.array_equal(bits(got[3][:n]), bits(w_pos))
    assert np.all(got[2][n:] == SENT_I) and np.all(got[3][n:] == np.float32(SENT_F))
    if owner is not None:
        assert np.array_equal(got[0], w_owner)
    return want


def orbit(n, distance=4.0, elevation=20.0, azimuth0=10.0):
    return render.orbit_path(n, (0.0, 0.0, 0.0), distance, elevation, azimuth0)


def noisy_sphere_maps(rng, poses, H, W, intr, spread=0.8):
    """Depths scattered around the distance to the origin, and accumulations uniform in [0, 1): about half fail a 0.5 threshold."""
    n = len(poses)
    dist = np.linalg.norm(poses[:, :, 3], axis=1)[:, None]
    depth = (dist + spread * rng.uniform(-1.0, 1.0, size=(n, H * W))).astype(np.float32)
    return depth, rng.uniform(size=(n, H * W)).astype(np.float32)


BOX = ((-1.5, -1.5, -1.5), 3.0)  # corner and side of the box the grids tile


def grid(cells):
    return (cells,) * 3, BOX[0], (np.float32(BOX[1] / cells),) * 3


# ---------------------------------------------------------------------------------------------- 1. the rule, clause by clause
H1, W1 = 3, 5
INTR1 = (4.0, 4.0, 2.5, 1.5)  # pixel (y, x) = (1, 2) looks straight down the camera's -z
POSE1 = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4]])[None]  # at z = 4, looking down -z: the centre ray is (0, 0, 4 - t)
WIDE = ((8, 8, 8), (-8.0, -8.0, -8.0), (2.0, 2.0, 2.0))  # holds every point of the 5 x 3 cases


def small(depth, acc=None, min_acc=0.5, edge=INF, frame=WIDE, owner=None):
    depth = np.float32(depth).reshape(1, H1 * W1)
    acc = None if acc is None else np.float32(acc).reshape(1, H1 * W1)
    want = check(owner, POSE1, H1, W1, INTR1, depth, acc, 0, *frame, min_acc, edge)
    return want[4].reshape(H1, W1)


def test_rule_depth_values():
    """0, negative, inf and NaN depths are no candidates; with the edge test off their finite neighbours stay, except beside a
    negative depth, where edge * min is -inf."""
    d = np.full((H1, W1), 2.0, np.float32)
    d[0, 0], d[0, 2], d[0, 4], d[2, 0], d[2, 4] = 0.0, -1.0, INF, NAN, -INF
    cand = small(d)
    assert not cand[0, 0] and not cand[0, 2] and not cand[0, 4] and not cand[2, 0] and not cand[2, 4]
    assert cand[1, 0] and cand[1, 4] and cand[2, 1] and cand[2, 3]  # beside 0 (inf * 0 is NaN), inf, NaN, -inf: kept
    assert not cand[0, 1] and not cand[0, 3] and not cand[1, 2]  # beside the negative depth
    assert cand.sum() == 4 + 3  # and the rest of the lower rows: (1, 1), (1, 3), (2, 2)


def test_rule_accumulation_threshold_and_nan():
    d = np.full((H1, W1), 2.0, np.float32)
    a = np.full((H1, W1), 0.9, np.float32)
    a[0, 0], a[0, 1], a[0, 2], a[1, 0] = 0.5, np.nextafter(np.float32(0.5), np.float32(0)), NAN, INF
    cand = small(d, a, min_acc=0.5)
    assert cand[0, 0] and not cand[0, 1] and not cand[0, 2] and cand[1, 0] and cand[2, 4]
    assert small(d, None).all()  # no accumulation map: every pixel
    assert small(d, a, min_acc=-INF).sum() == H1 * W1 - 1  # only the NaN fails
    # a neighbour's accumulation plays no part: the pixel beside a failed one is judged on depths alone
    assert small(d, a, min_acc=0.5, edge=0.05)[1, 1]


def test_rule_depth_edge():
    """A neighbour with a non-finite depth is ignored; a difference exactly at edge * min is kept, one ulp above is not."""
    d = np.full((H1, W1), 1.0, np.float32)
    d[1, 2] = INF
    d[0, 0] = NAN
    cand = small(d, edge=0.05)
    assert cand[0, 2] and cand[2, 2] and cand[1, 1] and cand[1, 3] and cand[0, 1] and cand[1, 0] and not cand[1, 2] and not cand[0, 0]
    d = np.full((H1, W1), 1.0, np.float32)
    d[0, :] = 1.5  # |1 - 1.5| == 0.5 * min(1, 1.5): exact in fp32
    assert small(d, edge=0.5).all()
    d[0, 3] = np.nextafter(np.float32(1.5), np.float32(2))
    cand = small(d, edge=0.5)
    assert not cand[0, 3] and not cand[1, 3] and cand[0, 1] and cand[1, 1] and cand.sum() == H1 * W1 - 2  # (0, 2) and (0, 4): 1.2e-7 < 0.75
    assert not small(d, edge=0.0)[0].any() and small(d, edge=0.0)[2].all()  # edge 0: any difference rejects
    assert small(d, edge=INF).all()


def test_rule_grid_faces():
    """The centre ray's point is (0, 0, 4 - D) exactly: on the lower face of the grid it is kept, on the upper face it is not."""
    d = np.full((H1, W1), 2.0, np.float32)
    low = ((4, 4, 4), (-1.0, -1.0, 2.0), (0.5, 0.5, 0.5))   # z in [2, 4): q_z == 0
    high = ((4, 4, 4), (-1.0, -1.0, 0.0), (0.5, 0.5, 0.5))  # z in [0, 2): q_z == 4 == nz
    ro, rd = device_rays(POSE1, H1, W1, INTR1)
    assert np.array_equal(rd[0, 1 * W1 + 2], np.float32([0, 0, -1])) and np.array_equal(ro[0, 0], np.float32([0, 0, 4]))
    assert small(d, frame=low)[1, 2] and not small(d, frame=high)[1, 2]
    x_low = ((4, 4, 4), (0.0, -1.0, 1.0), (0.5, 0.5, 0.5))   # x in [0, 2): q_x == 0
    x_high = ((4, 4, 4), (-2.0, -1.0, 1.0), (0.5, 0.5, 0.5))  # x in [-2, 0): q_x == 4
    assert small(d, frame=x_low)[1, 2] and not small(d, frame=x_high)[1, 2]
    one = ((1, 1, 1), (-0.25, -0.25, 1.75), (0.5, 0.5, 0.5))  # a single cell around the centre point
    assert small(d, frame=one).sum() == 1 and small(d, frame=one, owner=ref.new_owner((1, 1, 1)))[1, 2]


# ---------------------------------------------------------------------------------------------- 2. ragged sizes
@pytest.mark.parametrize("n,W,H", [(3, 37, 29), (2, 70, 50)])
@pytest.mark.parametrize("thin", [False, True])
def test_ragged_sizes(n, W, H, thin):
    """Neither side nor the pixel count is a multiple of 64 or 256; 13 and 28 tiles, the last one partial."""
    rng = np.random.default_rng(n * W + H)
    poses = orbit(n)
    intr = (1.2 * W, 1.2 * W, W / 2.0, H / 2.0)
    depth, acc = noisy_sphere_maps(rng, poses, H, W, intr)
    dims, o3, s3 = grid(12)
    owner = ref.new_owner(dims) if thin else None
    _, kept, _, _, cand, _ = check(owner, poses, H, W, intr, depth, acc, 0, dims, o3, s3, 0.5, 0.3)
    total = n * H * W
    assert total % 256 != 0 and W % 64 != 0 and kept % 64 != 0
    assert 0.1 * total < cand.sum() < 0.6 * total and (kept < cand.sum()) == thin


# ---------------------------------------------------------------------------------------------- 3. long calls
@pytest.mark.parametrize("W,H", [(300, 300), (520, 505)])
def test_every_pixel_of_a_long_call_in_order(W, H):
    """One view, every pixel a candidate, no owner: pixel_index is 0 .. H*W-1.  300 x 300 is 352 tiles of 256 pixels; 520 x 505 is
    more than the 1024 workgroups of a launch hold in one pass (262,144 pixels), so workgroups walk several tiles."""
    if W == 520:
        assert W * H > 1024 * 256
    poses = orbit(1)
    intr = (2.0 * W, 2.0 * W, W / 2.0, H / 2.0)
    depth = np.full((1, H * W), 4.0, np.float32)
    want = check(None, poses, H, W, intr, depth, None, 0, *grid(16), 0.5, 0.05)
    assert want[1] == H * W and np.array_equal(want[2], np.arange(H * W, dtype=np.int32))


# ---------------------------------------------------------------------------------------------- 4. thinning collisions
@pytest.mark.parametrize("cells", [2, 64])
def test_thinning_collisions_across_views(cells):
    """Two cameras 5 degrees apart see the same sphere: most cells hold pixels of both views, and of several rows of one view."""
    H, W = 29, 37
    intr = (3.0 * W, 3.0 * W, W / 2.0, H / 2.0)
    poses = render.orbit_path(72, (0.0, 0.0, 0.0), 4.0, 20.0)[:2]
    depth = np.stack([tref.sphere_depth(m, H, W, *intr, 0.8, 6.0) for m in poses])
    acc = (depth < np.float32(6.0)).astype(np.float32)
    dims, o3, s3 = grid(cells)
    owner, n, index, _, cand, cell = check(ref.new_owner(dims), poses, H, W, intr, depth, acc, 0, dims, o3, s3, 0.5, INF)
    g = ref.global_index(2, H, W, 0)
    occupied = np.unique(cell[cand])
    assert n == len(occupied) < cand.sum()
    assert index.tolist() == sorted(int(g[cand][cell[cand] == c].min()) for c in occupied)
    assert 1 < n <= cells ** 3
    both = [c for c in occupied if len({int(v) for v in (g[cand][cell[cand] == c] // (H * W))}) == 2]
    assert both and all(int(owner.reshape(-1)[c]) < H * W for c in both)  # seen by both views: the first one's pixel owns it


# ---------------------------------------------------------------------------------------------- 5. split calls
@pytest.mark.parametrize("thin", [True, False])
def test_five_views_equal_two_then_three(thin):
    H, W = 19, 23
    rng = np.random.default_rng(5)
    poses = orbit(5)
    intr = (1.5 * W, 1.5 * W, W / 2.0, H / 2.0)
    depth, acc = noisy_sphere_maps(rng, poses, H, W, intr, spread=0.5)
    dims, o3, s3 = grid(10)
    new = (lambda: ref.new_owner(dims)) if thin else (lambda: None)
    w_owner, n, index, pos, _, _ = check(new(), poses, H, W, intr, depth, acc, 0, dims, o3, s3, 0.4, 0.5)
    a = device_pair(new(), poses[:2], H, W, intr, depth[:2], acc[:2], 0, dims, o3, s3, 0.4, 0.5)
    b = device_pair(a[0], poses[2:], H, W, intr, depth[2:], acc[2:], 2, dims, o3, s3, 0.4, 0.5)  # owner as the first pair left it
    assert a[1] > 0 and b[1] > 0 and a[1] + b[1] == n
    assert np.array_equal(np.concatenate([a[2][:a[1]], b[2][:b[1]]]), index)
    assert np.array_equal(bits(np.concatenate([a[3][:a[1]], b[3][:b[1]]])), bits(pos))
    if thin:
        assert np.array_equal(b[0], w_owner)
        # the second pair against the reference on the pre-filled owner: cells the first two views took are respected
        check(a[0], poses[2:], H, W, intr, depth[2:], acc[2:], 2, dims, o3, s3, 0.4, 0.5)
        taken = a[0] != ref.NO_OWNER
        assert taken.any() and np.array_equal(b[0][taken], a[0][taken])


# ---------------------------------------------------------------------------------------------- 6. empty inputs
def test_empty_inputs():
    H, W = 9, 11
    poses = orbit(2)
    intr = (20.0, 20.0, W / 2.0, H / 2.0)
    dims, o3, s3 = grid(6)
    depth = np.full((2, H * W), 4.0, np.float32)
    # no candidate at all: the accumulation fails everywhere; then the depth; then the box
    for d, a, frame in ((depth, np.zeros_like(depth), (dims, o3, s3)), (np.full_like(depth, NAN), None, (dims, o3, s3)),
                        (depth, None, (dims, (50.0, 50.0, 50.0), s3))):
        owner, n, _, _, cand, _ = check(ref.new_owner(dims), poses, H, W, intr, d, a, 0, *frame, 0.5, 0.05)
        assert n == 0 and not cand.any() and np.all(owner == ref.NO_OWNER)
    # accumulation = NULL
    assert check(ref.new_owner(dims), poses, H, W, intr, depth, None, 0, dims, o3, s3, 0.5, 0.05)[1] > 0
    # n_views = 0: no launch, count 0, with and without pointers
    lib = _abi.load_library()
    n_points = torch.full((2,), SENT_I, device=DEV, dtype=torch.int32)
    owner = torch.full((6, 6, 6), ref.NO_OWNER, device=DEV, dtype=torch.int32)
    import ctypes as C

    f3 = (C.c_float * 3)(1, 1, 1)
    from reflect_sampling_nerf_amd import ops

    common = (0, None, H, W, 20.0, 20.0, 5.5, 4.5, None, None, 3, 6, 6, 6, f3, f3, 0.5, 0.05)
    assert lib.rsn_pointcloud_mark(*common, _abi.ptr(owner), ops._stream()) == 0
    assert lib.rsn_pointcloud_select(*common, _abi.ptr(owner), None, 0, _abi.ptr(n_points), None, None, None, ops._stream()) == 0
    torch.cuda.synchronize()
    assert n_points.tolist() == [0, SENT_I] and bool((owner == ref.NO_OWNER).all())  # no candidate count asked for: not written
    assert lib.rsn_pointcloud_select(*common, None, None, 0, _abi.ptr(n_points), C.c_void_p(n_points.data_ptr() + 4), None, None,
                                     ops._stream()) == 0
    torch.cuda.synchronize()
    assert n_points.tolist() == [0, 0]
    empty = torch.empty(0, H * W, device=DEV)
    got = pointcloud.select(None, dims, o3, s3, torch.empty(0, 3, 4, device=DEV), empty, empty, H, W, *intr, 0, 0.5, 0.05)
    assert got[0].tolist() == [0, 0] and got[1].numel() == 0
    with pytest.raises(_abi.RsnError):
        pointcloud.mark(None, dims, o3, s3, torch.from_numpy(poses).to(DEV), torch.from_numpy(depth).to(DEV), None, H, W, *intr, 0, 0.5, -1.0)


# ---------------------------------------------------------------------------------------------- 7. checkpoint -> PLY
RES, BOUNDS, SIDE, FOV_DEG = 24, (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), 16, 40.0
FOG_DEPTH = helpers.FOG_DEPTH


@pytest.fixture(scope="module")
def fog_checkpoint(tmp_path_factory):
    """A 4 x 64 field whose density head is a constant: a fog of sigma = ln 2 / 3.5, so every eval ray has its median depth about
    3.5 from its camera and an accumulation of about 0.69, wherever it looks (the construction of the TSDF export's fixture)."""
    return helpers.fog_checkpoint(tmp_path_factory.mktemp("fog") / "run", DEV)


def orbit_cameras():
    fx, fy, cx, cy = render.pinhole(SIDE, SIDE, math.radians(FOV_DEG))
    return {"c2w": render.orbit_path(4, (0.0, 0.0, 0.0), 4.0, 20.0), "width": SIDE, "height": SIDE, "fx": fx, "fy": fy, "cx": cx, "cy": cy}


def test_export_pointcloud_end_to_end(fog_checkpoint, tmp_path, capsys):
    ckpt, run = fog_checkpoint
    cams = orbit_cameras()
    res = pointcloud.export_pointcloud(ckpt, str(tmp_path / "a.ply"), cams, resolution=RES, bounds=BOUNDS, min_accumulation=0.5)
    assert set(res) == {"checkpoint", "step", "out", "points", "candidates", "views", "image", "resolution", "bounds", "spacing",
                        "min_accumulation", "edge", "thin", "mma", "seconds"}
    assert (res["views"], res["step"], res["image"], res["resolution"], res["thin"], res["edge"], res["mma"]) == (
        4, 5, [SIDE, SIDE], [RES] * 3, True, 0.05, "f32")
    assert res["spacing"] == [float(np.float32(3.0 / RES))] * 3
    assert set(res["seconds"]) == {"depth", "mark", "select", "attributes", "write"} and all(t >= 0 for t in res["seconds"].values())
    assert 0 < res["points"] <= res["candidates"] <= 4 * SIDE * SIDE
    vert, _ = ref.parse_ply_points(str(tmp_path / "a.ply"))
    assert len(vert["x"]) == res["points"]
    pos = np.stack([vert["x"], vert["y"], vert["z"]], 1)
    # the stages by hand on the checkpoint's model: the file's points, and where each one comes from
    model, _ = trainer.load_checkpoint(ckpt, None, DEV)
    model.field.set_mma_mode("f32")
    intr = (cams["fx"], cams["fy"], cams["cx"], cams["cy"])
    cloud = pointcloud.collect_points(model, cams["c2w"], SIDE, SIDE, *intr, BOUNDS, RES, 0.5, 0.05)
    assert np.array_equal(bits(cloud["positions"].cpu().numpy()), bits(pos)) and cloud["candidates"] == res["candidates"]
    index = cloud["pixel_index"].cpu().numpy().astype(np.int64)
    assert np.all(np.diff(index) > 0)
    depth, acc = [], []
    for m in cams["c2w"]:
        surf = model.get_surface_outputs_for_camera_ray_bundle(render.camera_rays(m, SIDE, SIDE, *intr, DEV))
        depth.append(surf["depth_fine"].reshape(-1).cpu().numpy())
        acc.append(surf["accumulation_fine"].reshape(-1).cpu().numpy())
    depth, acc = np.stack(depth), np.stack(acc)
    print(f"fog: depth {depth.min():.3f} .. {depth.max():.3f}, accumulation {acc.min():.3f} .. {acc.max():.3f}")
    assert depth.min() > 0 and 0.5 < acc.min() and acc.max() < 0.8  # what the thresholds 0.5 and 0.8 below rely on
    view, pix = index // (SIDE * SIDE), index % (SIDE * SIDE)
    dist = np.linalg.norm(pos.astype(np.float64) - cams["c2w"][view][:, :, 3].astype(np.float64), axis=1)
    assert np.abs(dist - depth[view, pix]).max() < 1e-5
    nrm = np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-5)
    # the reference on the re-rendered maps keeps the same pixels
    ro, rd = device_rays(cams["c2w"], SIDE, SIDE, intr)
    dims, o3, s3 = pointcloud.cell_frame(BOUNDS, RES)
    want = ref.mark_select(ref.new_owner(dims), ro, rd, depth, acc, SIDE, SIDE, 0, dims, o3, s3, 0.5, 0.05)
    assert np.array_equal(want[2], index) and np.array_equal(bits(want[3]), bits(pos)) and int(want[4].sum()) == res["candidates"]
    # the same through the command line: transforms-format poses with the size and the field of view
    frames = [{"file_path": f"./{i}", "transform_matrix": np.vstack([m, [[0, 0, 0, 1]]]).tolist()} for i, m in enumerate(cams["c2w"].astype(np.float64))]
    poses = tmp_path / "poses.json"
    poses.write_text(json.dumps({"camera_angle_x": math.radians(FOV_DEG), "w": SIDE, "h": SIDE, "frames": frames}))
    argv = ["export-pointcloud", "--ckpt", run, "--out", str(tmp_path / "b.ply"), "--resolution", str(RES), "--poses", str(poses)]
    assert trainer.main(argv) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    assert line == f"{res['points']} points from 4 depth maps 16 x 16 ({res['candidates']} candidates) -> {tmp_path / 'b.ply'}"
    blob = open(tmp_path / "a.ply", "rb").read()
    assert open(tmp_path / "b.ply", "rb").read() == blob  # two runs, one of them through the parser: identical bytes
    other = pointcloud.export_pointcloud(ckpt, str(tmp_path / "c.ply"), cams, resolution=RES, bounds=BOUNDS, views_per_launch=3, ray_chunk=100)
    assert open(tmp_path / "c.ply", "rb").read() == blob and other["points"] == res["points"] and other["candidates"] == res["candidates"]
    # a threshold above the fog's accumulation: a valid file without points
    none = pointcloud.export_pointcloud(ckpt, str(tmp_path / "d.ply"), cams, resolution=RES, bounds=BOUNDS, min_accumulation=0.8)
    assert none["points"] == 0 and none["candidates"] == 0 and len(ref.parse_ply_points(str(tmp_path / "d.ply"))[0]["x"]) == 0
    # --no-thin: every candidate
    assert trainer.main(argv[:4] + [str(tmp_path / "e.ply")] + argv[5:] + ["--no-thin"]) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    every, _ = ref.parse_ply_points(str(tmp_path / "e.ply"))
    assert len(every["x"]) == res["candidates"] >= res["points"]
    assert line.startswith(f"{res['candidates']} points from 4 depth maps 16 x 16 ({res['candidates']} candidates)")
