"""CPU-side checks of the point-cloud export: the contract of include/rsn.h, restated in numpy (tests/pointcloud_reference.py), on
analytic depth maps of a sphere -- the points lie on it, silhouette pixels go with the depth-edge test, thinning keeps the lowest
global pixel index of every cell, a call may be split between views --; the PLY writer; the command line; and the argument errors
of the three entry points, which return before any launch."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, pointcloud, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import pointcloud_reference as ref
from tests import tsdf_reference as tref

OK, INVALID, UNSUPPORTED = 0, -1, -2
RADIUS, DISTANCE, FAR = 0.8, 4.0, 6.0
H, W, FOCAL = 20, 24, 36.0  # the sphere's image has a radius of about 7 pixels
INTR = (FOCAL, FOCAL, W / 2.0, H / 2.0)
DIMS, ORIGIN, SPACING = (8, 8, 8), (-1.0, -1.0, -1.0), (0.25, 0.25, 0.25)


@pytest.fixture(scope="module")
def scene():
    """4 orbit cameras at distance 4 around a sphere of radius 0.8: rays and depth computed in fp64 and rounded; accumulation 1 on
    the sphere and 0 beside it, where the depth is the far end of the ray."""
    az = 2.0 * np.pi * np.arange(4) / 4 + 0.3
    el = math.radians(20.0)
    poses = np.stack([tref.look_at(DISTANCE * np.array([math.cos(el) * math.cos(a), math.cos(el) * math.sin(a), math.sin(el)])) for a in az])
    rays = [tref.pixel_rays(m, H, W, *INTR) for m in poses]
    o = np.stack([np.broadcast_to(r[0], (H * W, 3)) for r in rays]).astype(np.float32)
    d = np.stack([r[1] for r in rays]).astype(np.float32)
    depth = np.stack([tref.sphere_depth(m, H, W, *INTR, RADIUS, FAR) for m in poses])
    hit = depth < np.float32(FAR)
    return {"o": o, "d": d, "depth": depth, "acc": hit.astype(np.float32), "hit": hit}


def run(scene, views, view0, owner, edge, min_acc=0.5):
    v = slice(*views)
    return ref.mark_select(owner, scene["o"][v], scene["d"][v], scene["depth"][v], scene["acc"][v], H, W, view0, DIMS, ORIGIN, SPACING,
                           min_acc, edge)


def silhouette(hit):
    """Pixels on the sphere with a 4-neighbour beside it."""
    m = hit.reshape(-1, H, W)
    off = np.zeros_like(m)
    off[:, 1:, :] |= ~m[:, :-1, :]
    off[:, :-1, :] |= ~m[:, 1:, :]
    off[:, :, 1:] |= ~m[:, :, :-1]
    off[:, :, :-1] |= ~m[:, :, 1:]
    return (m & off).reshape(hit.shape)


def test_points_lie_on_the_sphere_and_silhouette_pixels_go_with_the_edge_test(scene):
    sil = silhouette(scene["hit"])
    assert sil.sum() > 4 * 20 and (scene["hit"] & ~sil).sum() > 4 * 50
    _, n, index, pos, cand, _ = run(scene, (0, 4), 0, None, 0.05)
    assert 0 < n == cand.sum() and not cand[sil].any() and not cand[~scene["hit"]].any()
    assert np.abs(np.linalg.norm(pos.astype(np.float64), axis=1) - RADIUS).max() < 1e-5
    assert np.array_equal(index, np.flatnonzero(cand.reshape(-1)))  # ascending global pixel index
    _, n_inf, _, pos_inf, cand_inf, _ = run(scene, (0, 4), 0, None, np.inf)
    assert cand_inf[sil].all() and np.array_equal(cand_inf, scene["hit"]) and n_inf > n
    assert np.abs(np.linalg.norm(pos_inf.astype(np.float64), axis=1) - RADIUS).max() < 1e-5
    # without an accumulation map the rays beside the sphere are candidates as far as the box reaches: none, 6 away from the camera
    c, _, _ = ref.candidates(scene["o"], scene["d"], scene["depth"], None, H, W, DIMS, ORIGIN, SPACING, 0.5, np.inf)
    assert np.array_equal(c, scene["hit"])


def test_thinning_keeps_the_lowest_pixel_index_of_every_cell(scene):
    owner, n, index, pos, cand, cell = run(scene, (0, 4), 0, ref.new_owner(DIMS), 0.05)
    g = ref.global_index(4, H, W, 0)
    occupied = np.unique(cell[cand])
    assert 1 < len(occupied) == n < cand.sum()  # views overlap and cells hold several pixels: thinning drops some
    lowest = {int(c): int(g[cand][cell[cand] == c].min()) for c in occupied}
    assert sorted(lowest.values()) == index.tolist()
    flat = owner.reshape(-1)
    assert all(flat[c] == lowest[c] for c in lowest) and (flat != ref.NO_OWNER).sum() == n
    assert np.array_equal(pos, ref.candidates(scene["o"], scene["d"], scene["depth"], scene["acc"], H, W, DIMS, ORIGIN, SPACING, 0.5,
                                              0.05)[1].reshape(-1, 3)[index])


@pytest.mark.parametrize("thin", [True, False])
def test_four_views_at_once_equal_one_then_three(scene, thin):
    owner, n, index, pos, _, _ = run(scene, (0, 4), 0, ref.new_owner(DIMS) if thin else None, 0.05)
    o1, n1, i1, p1, _, _ = run(scene, (0, 1), 0, ref.new_owner(DIMS) if thin else None, 0.05)
    o2, n2, i2, p2, _, _ = run(scene, (1, 4), 1, o1, 0.05)
    assert n1 > 0 and n2 > 0 and n1 + n2 == n
    assert np.array_equal(np.concatenate([i1, i2]), index)
    assert np.array_equal(np.concatenate([p1, p2]).view(np.uint32), pos.view(np.uint32))
    if thin:
        assert np.array_equal(o2, owner)


# ---------------------------------------------------------------------------------------------- the writer
def test_ply_points_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    P = 37
    cloud = {"positions": rng.normal(size=(P, 3)).astype(np.float32), "pred_normals": rng.normal(size=(P, 3)).astype(np.float32),
             "diff": rng.uniform(-0.2, 1.2, size=(P, 3)).astype(np.float32), "roughness": rng.uniform(size=P).astype(np.float32),
             "tint": rng.uniform(size=(P, 3)).astype(np.float32), "pixel_index": np.arange(P, dtype=np.int32)}
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "sub" / "b.ply")
    assert pointcloud.write_ply_points(a, cloud) == a
    import torch

    pointcloud.write_ply_points(b, {k: torch.from_numpy(v) for k, v in cloud.items()})
    blob = open(a, "rb").read()
    assert open(b, "rb").read() == blob and not list(tmp_path.glob("*.tmp"))
    header = blob[:blob.index(b"end_header\n")].decode("ascii")
    assert "element face" not in header and f"element vertex {P}" in header
    vert, lines = ref.parse_ply_points(a)
    assert tuple(vert) == mesh.PLY_VERTEX_DTYPE.names
    for c, (p, q, t) in enumerate((("x", "nx", "tint_r"), ("y", "ny", "tint_g"), ("z", "nz", "tint_b"))):
        assert np.array_equal(vert[p], cloud["positions"][:, c]) and np.array_equal(vert[q], cloud["pred_normals"][:, c])
        assert np.array_equal(vert[t], cloud["tint"][:, c])
    assert np.array_equal(vert["roughness"], cloud["roughness"])
    want = np.floor(np.clip(cloud["diff"], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), want) and want.min() == 0 and want.max() == 255
    empty = {k: v[:0] for k, v in cloud.items()}
    vert0, _ = ref.parse_ply_points(pointcloud.write_ply_points(str(tmp_path / "e.ply"), empty))
    assert len(vert0["x"]) == 0


def test_cell_frame_tiles_the_bounds():
    n, o, s = pointcloud.cell_frame((-1.5, -1.0, 0.0, 1.5, 1.0, 4.0), (6, 4, 1))
    assert n == (6, 4, 1) and o.dtype == np.float32 and np.array_equal(o, np.float32([-1.5, -1.0, 0.0]))
    assert np.array_equal(s, np.float32([0.5, 0.5, 4.0]))
    with pytest.raises(ValueError):
        pointcloud.cell_frame((0, 0, 0, 1, 1, 1), 0)
    with pytest.raises(ValueError):
        pointcloud.cell_frame((0, 0, 0, 1, 0, 1), 4)


# ---------------------------------------------------------------------------------------------- command line
def _poses_file(tmp_path, n=5, w=16, h=12, angle=0.8):
    frames = [{"file_path": f"./f{i}", "transform_matrix": np.vstack([tref.look_at((3.0 * np.cos(i), 3.0 * np.sin(i), 1.0)), [[0, 0, 0, 1]]]).tolist()}
              for i in range(n)]
    path = tmp_path / "poses.json"
    path.write_text(json.dumps({"camera_angle_x": angle, "w": w, "h": h, "frames": frames}))
    return str(path)


def test_cli_of_export_pointcloud(tmp_path, capsys):
    base = ["export-pointcloud", "--ckpt", "run", "--out", "c.ply"]
    poses = _poses_file(tmp_path)
    ap = trainer.build_parser()
    a = ap.parse_args(base + ["--poses", poses])
    assert (a.resolution, a.min_accumulation, a.edge, a.no_edge, a.no_thin, a.max_views, a.downscale, a.split, a.mma) == (
        512, 0.5, 0.05, False, False, None, 1, "train", "f32")
    assert (pointcloud.DEFAULT_RESOLUTION, pointcloud.DEFAULT_MIN_ACCUMULATION, pointcloud.DEFAULT_EDGE) == (512, 0.5, 0.05)
    s = trainer.resolve_pointcloud_args(ap, a)
    assert s["cameras"]["c2w"].shape == (5, 3, 4) and (s["cameras"]["width"], s["cameras"]["height"]) == (16, 12)
    assert (s["resolution"], s["bounds"], s["min_accumulation"], s["edge"], s["thin"], s["ray_chunk"], s["chunk"]) == (
        512, mesh.DEFAULT_BOUNDS, 0.5, 0.05, True, mesh.DEFAULT_RAY_CHUNK, mesh.DEFAULT_CHUNK)
    a = ap.parse_args(base + ["--poses", poses, "--max-views", "3", "--downscale", "2", "--no-edge", "--no-thin", "--resolution", "64",
                              "--min-accumulation", "0.9", "--bounds", "-1", "-1", "-1", "1", "1", "2", "--ray-chunk", "100"])
    s = trainer.resolve_pointcloud_args(ap, a)
    assert s["edge"] == math.inf and s["thin"] is False and s["resolution"] == 64 and s["bounds"] == (-1.0, -1.0, -1.0, 1.0, 1.0, 2.0)
    assert s["cameras"]["c2w"].shape == (3, 3, 4) and (s["cameras"]["width"], s["cameras"]["height"]) == (8, 6) and s["ray_chunk"] == 100
    # the cameras are the ones export-mesh --method tsdf resolves from the same flags
    mesh_cam = trainer.resolve_export_cameras(ap, ap.parse_args(["export-mesh", "--ckpt", "run", "--out", "m.ply", "--method", "tsdf",
                                                                 "--poses", poses, "--max-views", "3", "--downscale", "2"]))
    assert all(np.array_equal(mesh_cam[k], s["cameras"][k]) for k in mesh_cam)

    def fails(argv, *words):
        with pytest.raises(SystemExit):
            trainer.main(argv)
        err = capsys.readouterr().err
        assert all(w in err for w in words), err

    fails(base, "export-pointcloud", "--data", "--poses")  # no cameras
    fails(base + ["--poses", poses, "--data", str(tmp_path)], "--data", "--poses", "one of them")
    fails(base + ["--poses", poses, "--edge", "-1"], "--edge")
    fails(base + ["--edge", "-1"], "--edge")  # settled by the command line alone: before the cameras are looked for
    fails(base + ["--poses", poses, "--edge", "nan"], "--edge")
    fails(base + ["--poses", poses, "--resolution", "0"], "--resolution")
    fails(base + ["--poses", poses, "--resolution", "513"], "--resolution")
    fails(base + ["--poses", poses, "--edge", "0.1", "--no-edge"], "--no-edge")
    fails(base + ["--poses", poses, "--min-accumulation", "nan"], "--min-accumulation")
    fails(base + ["--poses", poses, "--downscale", "0"], "--downscale")
    fails(base + ["--poses", poses, "--bounds", "0", "0", "0", "1", "1", "0"], "--bounds")
    # export-mesh says what it said
    mesh_base = ["export-mesh", "--ckpt", "run", "--out", "m.ply"]
    fails(mesh_base + ["--method", "tsdf"], "export-mesh: --method tsdf needs cameras: give --data DIR or --poses FILE.json (one of them)")
    fails(mesh_base + ["--method", "tsdf", "--poses", poses, "--downscale", "0"], "export-mesh: --downscale and --max-views must be >= 1")
    fails(mesh_base + ["--method", "tsdf", "--poses", poses, "--trunc", "0"], "export-mesh: --trunc 0.0: need a finite value above 0")
    fails(mesh_base + ["--poses", poses], "export-mesh: --poses need(s) --method tsdf")
    sub = [act for act in ap._actions if hasattr(act, "choices") and act.choices and "export-pointcloud" in act.choices]
    text = " ".join(sub[0].choices["export-pointcloud"].format_help().split())
    assert text.count("not measured on a scene") >= 3


# ---------------------------------------------------------------------------------------------- the entry points
@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def test_symbols_are_bound_and_argument_errors_return_before_any_launch(lib):
    """Made-up pointers: a call that reached the device would fault, and there is no device here anyway."""
    for name in ("rsn_pointcloud_workspace_bytes", "rsn_pointcloud_mark", "rsn_pointcloud_select"):
        assert name in _abi.EXPORTED_SYMBOLS
    assert lib.rsn_abi_version() == 18
    p = C.c_void_p(0x1000)
    f3 = (C.c_float * 3)(1, 1, 1)
    nan, inf = float("nan"), float("inf")

    def args(kw):
        a = dict(n=1, c2w=p, h=8, w=8, fx=8.0, fy=8.0, depth=p, acc=p, view0=0, nx=4, ny=4, nz=4, o=f3, s=f3, min_acc=0.5, edge=0.05)
        a.update(kw)
        return (a["n"], a["c2w"], a["h"], a["w"], a["fx"], a["fy"], 4.0, 4.0, a["depth"], a["acc"], a["view0"], a["nx"], a["ny"], a["nz"],
                a["o"], a["s"], a["min_acc"], a["edge"])

    def mark(owner=p, **kw):
        return lib.rsn_pointcloud_mark(*args(kw), owner, None)

    def select(ws=p, ws_bytes=1 << 20, n_points=p, n_cand=p, index=p, pos=p, **kw):
        return lib.rsn_pointcloud_select(*args(kw), p, ws, ws_bytes, n_points, n_cand, index, pos, None)

    bad3 = lambda *v: (C.c_float * 3)(*v)  # noqa: E731
    shared = (dict(nx=0), dict(ny=0), dict(nz=-1), dict(h=0), dict(w=0), dict(n=-1), dict(view0=-1), dict(h=2 ** 16, w=2 ** 15),
              dict(view0=2 ** 25 - 1, h=8, w=8), dict(c2w=None), dict(depth=None), dict(o=None), dict(s=None),
              dict(s=bad3(1, 0, 1)), dict(s=bad3(1, 1, -1)), dict(s=bad3(inf, 1, 1)), dict(s=bad3(1, nan, 1)), dict(o=bad3(0, inf, 0)),
              dict(o=bad3(nan, 0, 0)), dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=inf), dict(min_acc=nan), dict(edge=nan),
              dict(edge=-0.5), dict(edge=-inf))
    for call in (mark, select):
        for kw in shared:
            assert call(**kw) == INVALID, (call.__name__, kw)
            assert lib.rsn_last_error()
        assert call(nx=1024, ny=1024, nz=1024) == UNSUPPORTED and b"2^27" in lib.rsn_last_error()
        assert call(nx=513, ny=512, nz=512) == UNSUPPORTED
        # no views: nothing to launch (select still sets its count: not callable without a device), and the index bound is met
        assert call(n=-1, view0=2 ** 25) == INVALID
    assert mark(n=0) == OK and mark(n=0, c2w=None, depth=None, acc=None, o=None, s=None, owner=None) == OK
    assert mark(n=0, view0=2 ** 25 - 1, h=8, w=8) == OK and mark(n=0, view0=2 ** 25, h=8, w=8) == INVALID  # (view0 + 0) * 64 <= 2^31 - 1
    assert mark(n=0, nx=512, ny=512, nz=512) == OK
    assert mark(owner=None) == OK  # no thinning: nothing to record, nothing launched
    assert mark(owner=None, edge=inf, acc=None, min_acc=-inf) == OK
    for kw in (dict(ws=None), dict(index=None), dict(pos=None), dict(n_points=None), dict(n=0, n_points=None)):
        assert select(**kw) == INVALID, kw
    need = lib.rsn_pointcloud_workspace_bytes(1, 8, 8)
    assert need >= 64 + 8 and select(ws_bytes=need - 1) == -4 and select(ws_bytes=need - 1, n_cand=None) == -4 and b"needed" in lib.rsn_last_error()
    assert select(ws=C.c_void_p(0x1001)) == INVALID  # alignment
    # the size function: host only
    assert lib.rsn_pointcloud_workspace_bytes(0, 8, 8) > 0
    assert lib.rsn_pointcloud_workspace_bytes(8, 800, 800) >= 8 * 800 * 800 + 8 * (8 * 800 * 800 // 256)
    for shape in ((-1, 8, 8), (1, 0, 8), (1, 8, 0), (2, 2 ** 15, 2 ** 15), (1, 2 ** 16, 2 ** 15)):
        assert lib.rsn_pointcloud_workspace_bytes(*shape) == 0 and b"pointcloud" in lib.rsn_last_error()
    assert lib.rsn_pointcloud_workspace_bytes(1, 2 ** 16, 2 ** 15 - 1) > 2 ** 31 - 2 ** 16
