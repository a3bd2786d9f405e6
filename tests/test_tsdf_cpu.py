"""CPU-side checks of the TSDF mesh export: the fusion contract of include/rsn.h, restated in numpy (tests/tsdf_reference.py), gives
a single closed shell on analytic depth maps of a sphere once the unobserved part is dropped; mesh.drop_unobserved on CPU tensors is
that filter; the entry point is bound and refuses bad arguments before any launch; the command line knows the new flags."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import mesh_reference as mref
from tests import tsdf_reference as ref

OK, INVALID, UNSUPPORTED = 0, -1, -2
RADIUS, DISTANCE, FAR = 0.8, 3.0, 6.0
BOX = 1.2  # the grid spans [-BOX, BOX]^3: the sphere plus half its radius, so that free space surrounds it on every side
# (grid vertices per axis, views, image side): the configurations of the experiment the contract's defaults come from
CONFIGS = ((16, 6, 48), (24, 14, 64), (32, 26, 96))


def sphere_fusion(res, n_views, side, trunc_spacings):
    """-> (mesh before the filter, after it, weight, spacing h) of the reference pipeline on the analytic sphere."""
    n = (res, res, res)
    h = np.float32(2.0 * BOX / (res - 1))
    o, s = np.float32([-BOX] * 3), np.float32([h] * 3)
    f, c = 1.2 * side, side / 2.0
    poses = np.stack([ref.look_at(DISTANCE * d) for d in ref.view_directions(n_views)])
    depth = np.stack([ref.sphere_depth(m, side, side, f, f, c, c, RADIUS, FAR) for m in poses])
    T, W = ref.integrate(np.zeros(n, np.float32), np.zeros(n, np.float32), o, s, poses, side, side, f, f, c, c, depth,
                         trunc_spacings * h, 0.0)
    full = mref.extract(ref.tsdf_volume(T, W, 1.0), 0.0, o, s)
    return full, ref.drop_unobserved(full, W, n, 1.0), W, float(h)


@pytest.fixture(scope="module")
def fused():
    return {(cfg, t): sphere_fusion(*cfg, t) for cfg in CONFIGS for t in (3.0, 4.0)}


@pytest.mark.parametrize("trunc_spacings", [3.0, 4.0])
@pytest.mark.parametrize("config", CONFIGS)
def test_sphere_fuses_to_one_closed_shell(fused, config, trunc_spacings):
    full, kept, W, h = fused[(config, trunc_spacings)]
    assert mref.euler_characteristic(kept["triangles"]) == 2
    assert len(mref.unmatched_edges(kept["triangles"])) == 0
    assert len(np.unique(kept["triangles"])) == len(kept["positions"])  # no unreferenced vertex survives
    err = np.abs(np.linalg.norm(kept["positions"], axis=1) - RADIUS).max() / h
    print(f"{config} trunc {trunc_spacings} h: {len(full['triangles'])} -> {len(kept['triangles'])} triangles, "
          f"largest distance from the sphere {err:.3f} spacings")
    assert err <= 1.0
    assert len(kept["triangles"]) < len(full["triangles"])  # the filter is what removes the inner shell
    assert mref.signed_volume(kept["positions"], kept["triangles"]) > 0  # normals point out of the object


def test_without_the_filter_there_is_a_second_shell(fused):
    full, kept, _, h = fused[(CONFIGS[1], 4.0)]
    assert len(mref.unmatched_edges(full["triangles"])) == 0 and mref.euler_characteristic(full["triangles"]) == 4
    inner = RADIUS - np.linalg.norm(full["positions"], axis=1).min()
    assert inner / h > 2.0  # well inside the object, where the observed band ends


@pytest.mark.parametrize("min_weight", [1.0, 3.0])
def test_drop_unobserved_on_cpu_tensors_equals_the_reference(fused, min_weight):
    full, _, W, _ = fused[(CONFIGS[0], 3.0)]
    res = CONFIGS[0][0]
    want = ref.drop_unobserved(full, W, (res, res, res), min_weight)
    m = {"positions": torch.from_numpy(full["positions"].astype(np.float32)), "vert_key": torch.from_numpy(full["vert_key"].astype(np.int32)),
         "triangles": torch.from_numpy(full["triangles"].astype(np.int32))}
    got = mesh.drop_unobserved(m, torch.from_numpy(W), (res, res, res), min_weight)
    assert got["triangles"].dtype == torch.int32 and got["vert_key"].dtype == torch.int32
    assert 0 < len(want["triangles"]) < len(full["triangles"])
    assert np.array_equal(got["triangles"].numpy(), want["triangles"])
    assert np.array_equal(got["vert_key"].numpy(), want["vert_key"])
    assert np.array_equal(got["positions"].numpy(), want["positions"].astype(np.float32))
    vol = mesh.tsdf_volume(torch.tensor([0.5, -0.25, 0.5, -0.0]), torch.tensor([1.0, 3.0, 0.0, 2.0]), min_weight)
    assert np.array_equal(vol.numpy(), ref.tsdf_volume(np.float32([0.5, -0.25, 0.5, -0.0]), np.float32([1.0, 3.0, 0.0, 2.0]), min_weight))
    assert vol.tolist()[2] == -1.0


def test_an_empty_mesh_and_a_fully_observed_one_pass_through():
    empty = {"positions": torch.zeros(0, 3), "vert_key": torch.zeros(0, dtype=torch.int32), "triangles": torch.zeros(0, 3, dtype=torch.int32)}
    got = mesh.drop_unobserved(empty, torch.ones(3, 3, 3), (3, 3, 3))
    assert got["positions"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["vert_key"].shape == (0,)
    o, s = (-1.0, -1.0, -1.0), (0.25, 0.25, 0.25)
    full = mref.extract(mref.sphere((9, 9, 9), o, s, (0, 0, 0), 0.6), 0.0, o, s)
    m = {k: torch.from_numpy(v) for k, v in full.items()}
    got = mesh.drop_unobserved(m, torch.ones(9, 9, 9), (9, 9, 9))
    assert all(torch.equal(got[k], m[k]) for k in m)


# ---------------------------------------------------------------------------------------------- the entry point
@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def test_symbol_is_bound_and_argument_errors_return_before_any_launch(lib):
    """Made-up pointers: a call that reached the device would fault, and there is no device here anyway."""
    assert "rsn_tsdf_integrate" in _abi.EXPORTED_SYMBOLS and lib.rsn_abi_version() == 18
    p = C.c_void_p(0x1000)
    f3 = (C.c_float * 3)(1, 1, 1)
    nan, inf = float("nan"), float("inf")

    def call(nx=4, ny=4, nz=4, o=f3, s=f3, n=1, c2w=p, h=8, w=8, fx=8.0, fy=8.0, depth=p, trunc=0.5, near=0.0, t=p, wt=p):
        return lib.rsn_tsdf_integrate(nx, ny, nz, o, s, n, c2w, h, w, fx, fy, 4.0, 4.0, depth, trunc, near, t, wt, None)

    for kw in (dict(nx=1), dict(ny=1), dict(nz=0), dict(h=0), dict(w=0), dict(h=2 ** 16, w=2 ** 15), dict(n=-1), dict(o=None),
               dict(s=None), dict(c2w=None), dict(depth=None), dict(t=None), dict(wt=None), dict(trunc=0.0), dict(trunc=-1.0),
               dict(trunc=nan), dict(trunc=inf), dict(near=nan), dict(near=inf), dict(fx=0.0), dict(fy=0.0), dict(fx=nan), dict(fy=inf)):
        assert call(**kw) == INVALID, kw
        assert lib.rsn_last_error()
    assert call(h=2 ** 16, w=2 ** 15 - 1, n=0) == OK  # H * W = 2^31 - 2^16 is allowed
    assert call(nx=1024, ny=1024, nz=1024) == UNSUPPORTED and b"2^27" in lib.rsn_last_error()
    assert call(nx=513, ny=512, nz=512) == UNSUPPORTED
    # no views: nothing to launch, and then no pointer is needed
    assert call(n=0) == OK and call(n=0, o=None, s=None, c2w=None, depth=None, t=None, wt=None) == OK
    assert call(nx=512, ny=512, nz=512, n=0) == OK


# ---------------------------------------------------------------------------------------------- command line
def _poses_file(tmp_path, n=5, w=16, h=12, angle=0.8):
    frames = [{"file_path": f"./f{i}", "transform_matrix": np.vstack([ref.look_at((3.0 * np.cos(i), 3.0 * np.sin(i), 1.0)), [[0, 0, 0, 1]]]).tolist()}
              for i in range(n)]
    path = tmp_path / "poses.json"
    path.write_text(json.dumps({"camera_angle_x": angle, "w": w, "h": h, "frames": frames}))
    return str(path)


def test_cli_flags_of_the_tsdf_route(tmp_path, capsys):
    base = ["export-mesh", "--ckpt", "run", "--out", "m.ply"]
    ap = trainer.build_parser()
    a = ap.parse_args(base)
    assert (a.method, a.data, a.split, a.poses, a.scale_factor, a.max_views, a.downscale, a.trunc, a.min_weight) == (
        "density", None, "train", None, 1.0, None, 1, None, None)
    assert trainer.resolve_export_cameras(ap, a) is None
    assert mesh.DEFAULT_MIN_WEIGHT == 1.0 and mesh.DEFAULT_TRUNC_SPACINGS == 4.0
    poses = _poses_file(tmp_path)
    a = ap.parse_args(base + ["--method", "tsdf", "--poses", poses, "--max-views", "3", "--downscale", "2", "--trunc", "0.05",
                              "--min-weight", "2", "--scale-factor", "0.5"])
    assert (a.method, a.max_views, a.downscale, a.trunc, a.min_weight) == ("tsdf", 3, 2, 0.05, 2.0)
    cam = trainer.resolve_export_cameras(ap, a)
    assert (cam["width"], cam["height"]) == (8, 6) and cam["c2w"].shape == (3, 3, 4)
    f = 0.5 * 16 / np.tan(0.4)
    assert np.allclose([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], [f / 2, f / 2, 4.0, 3.0], rtol=1e-12)
    all5 = trainer.resolve_export_cameras(ap, ap.parse_args(base + ["--method", "tsdf", "--poses", poses, "--scale-factor", "0.5"]))
    assert all5["c2w"].shape == (5, 3, 4) and (all5["width"], all5["height"]) == (16, 12)
    assert np.array_equal(cam["c2w"], all5["c2w"][[0, 1, 3]])  # evenly spaced: floor(i * 5 / 3)
    assert np.allclose(np.linalg.norm(all5["c2w"][:, :, 3], axis=1), 0.5 * np.sqrt(10.0), rtol=1e-6)  # --scale-factor
    # a scene directory: the size comes from the first image's header
    from PIL import Image

    scene = tmp_path / "scene"
    scene.mkdir()
    meta = json.loads(open(poses).read())
    del meta["w"], meta["h"]
    (scene / "transforms_train.json").write_text(json.dumps(meta))
    Image.new("RGBA", (20, 10)).save(scene / "f0.png")
    cam = trainer.resolve_export_cameras(ap, ap.parse_args(base + ["--method", "tsdf", "--data", str(scene)]))
    assert (cam["width"], cam["height"], cam["c2w"].shape) == (20, 10, (5, 3, 4))

    def fails(extra, word):
        with pytest.raises(SystemExit):
            trainer.main(base + extra)
        assert word in capsys.readouterr().err

    fails(["--method", "tsdf"], "cameras")  # no cameras
    fails(["--method", "tsdf", "--poses", poses, "--data", str(scene)], "one of them")
    fails(["--method", "tsdf", "--poses", poses, "--iso", "3"], "--iso")
    fails(["--poses", poses], "--method tsdf")  # the tsdf flags without the method
    fails(["--trunc", "0.1"], "--method tsdf")
    fails(["--method", "tsdf", "--poses", poses, "--trunc", "0"], "--trunc")
    fails(["--method", "tsdf", "--poses", poses, "--downscale", "0"], "--downscale")
    fails(["--method", "voxels"], "invalid choice")
    sub = [act for act in ap._actions if hasattr(act, "choices") and act.choices and "export-mesh" in act.choices]
    text = " ".join(sub[0].choices["export-mesh"].format_help().split())
    assert "--method" in text and text.count("not measured on a scene") >= 2
