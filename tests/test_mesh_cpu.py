"""CPU-side checks of the mesh export: the three C entry points are bound and refuse bad arguments before any launch, the PLY
writer round-trips through a parser written here, the CLI knows `export-mesh`, and the numpy reference the GPU tests compare
against (tests/mesh_reference.py) produces closed, outward-oriented, second-order accurate surfaces on analytic volumes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import mesh_reference as ref
from tests.mesh_reference import parse_ply

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


def test_symbols_are_bound_and_abi_is_18(lib):
    for name in ("rsn_mesh_workspace_bytes", "rsn_mesh_count", "rsn_mesh_emit"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(r"#define RSN_ABI_VERSION 18\b", header)
    assert _abi.RSN_ABI_VERSION == 18 and lib.rsn_abi_version() == 18


def test_workspace_bytes_monotone_and_limits(lib):
    sizes = [lib.rsn_mesh_workspace_bytes(n, n, n) for n in (2, 3, 5, 17, 64, 161, 256, 512)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    for n, s in zip((64, 161, 256, 512), sizes[4:]):  # about 5 bytes per grid point, never more than 9
        assert 5 * n ** 3 <= s <= 9 * n ** 3
    assert lib.rsn_mesh_workspace_bytes(7, 5, 3) <= lib.rsn_mesh_workspace_bytes(7, 5, 4) <= lib.rsn_mesh_workspace_bytes(8, 5, 4)
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (-3, 4, 4)):
        assert lib.rsn_mesh_workspace_bytes(*dims) == 0
        assert b"at least 2" in lib.rsn_last_error()
    for dims in ((513, 512, 512), (2 ** 14, 2 ** 14, 2), (2 ** 30, 2 ** 30, 2 ** 30)):
        assert lib.rsn_mesh_workspace_bytes(*dims) == 0
        assert b"2^27" in lib.rsn_last_error()
    assert lib.rsn_mesh_workspace_bytes(512, 512, 512) > 0 and lib.rsn_mesh_workspace_bytes(2 ** 26, 2, 1) == 0


def test_argument_errors_return_before_any_launch(lib):
    """Made-up pointers: a call that reached the device would fault, and there is no device here anyway."""
    p = C.c_void_p(0x1000)
    o3, s3 = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    need = lib.rsn_mesh_workspace_bytes(4, 4, 4)
    count = lambda nx=4, ny=4, nz=4, vol=p, ws=p, nb=need, cnt=p: lib.rsn_mesh_count(nx, ny, nz, vol, 0.5, ws, nb, cnt, None)  # noqa: E731
    assert count(nx=1) == INVALID and count(nz=0) == INVALID
    assert count(nx=1024, ny=1024, nz=1024) == UNSUPPORTED
    assert count(vol=None) == INVALID and count(ws=None) == INVALID and count(cnt=None) == INVALID
    assert count(nb=need - 1) == WORKSPACE and b"needed" in lib.rsn_last_error()
    assert count(ws=C.c_void_p(0x1001)) == INVALID

    def emit(nx=4, ny=4, nz=4, vol=p, o=o3, s=s3, ws=p, nb=need, mv=8, mt=8, pos=p, key=p, tri=p):
        return lib.rsn_mesh_emit(nx, ny, nz, vol, 0.5, o, s, ws, nb, mv, mt, pos, key, tri, None)

    assert emit(ny=1) == INVALID and emit(nx=1024, ny=1024, nz=1024) == UNSUPPORTED
    assert emit(vol=None) == INVALID and emit(ws=None) == INVALID and emit(o=None) == INVALID and emit(s=None) == INVALID
    assert emit(mv=-1) == INVALID and emit(mt=-1) == INVALID
    assert emit(pos=None) == INVALID and emit(tri=None) == INVALID
    assert emit(nb=need - 1) == WORKSPACE
    assert emit(s=(C.c_float * 3)(1, 0, 1)) == INVALID and emit(s=(C.c_float * 3)(1, -1, 1)) == INVALID
    assert emit(s=(C.c_float * 3)(1, float("nan"), 1)) == INVALID and emit(o=(C.c_float * 3)(0, float("inf"), 0)) == INVALID
    assert emit(o=(C.c_float * 3)(3e38, 0, 0), s=(C.c_float * 3)(3e38, 1, 1)) == INVALID  # the far corner overflows
    # zero capacities: OK, nothing to launch, output pointers may be NULL
    assert emit(mv=0, mt=0, pos=None, key=None, tri=None) == OK


# ---------------------------------------------------------------------------------------------- PLY
def test_ply_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    V, T = 11, 7
    m = {"positions": rng.normal(size=(V, 3)).astype(np.float32), "triangles": rng.integers(0, V, size=(T, 3)).astype(np.int32),
         "pred_normals": rng.normal(size=(V, 3)).astype(np.float32), "diff": rng.uniform(-0.2, 1.2, size=(V, 3)).astype(np.float32),
         "roughness": rng.uniform(size=V).astype(np.float32), "tint": rng.uniform(size=(V, 3)).astype(np.float32)}
    m["diff"][0] = (0.0, 1.0, 127.5 / 255.0)  # the quantiser's corners: 0, 255, and a tie that rounds up to 128
    path = mesh.write_ply(str(tmp_path / "sub" / "m.ply"), m)
    vert, faces, lines = parse_ply(path)
    assert [ln for ln in lines if ln.startswith("property")] == [
        "property float x", "property float y", "property float z", "property float nx", "property float ny",
        "property float nz", "property uchar red", "property uchar green", "property uchar blue", "property float roughness",
        "property float tint_r", "property float tint_g", "property float tint_b", "property list uchar int vertex_indices"]
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), m["positions"])
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), m["pred_normals"])
    assert np.array_equal(np.stack([vert["tint_r"], vert["tint_g"], vert["tint_b"]], 1), m["tint"])
    assert np.array_equal(vert["roughness"], m["roughness"]) and np.array_equal(faces, m["triangles"])
    want = np.floor(np.clip(m["diff"].astype(np.float64), 0, 1) * 255 + 0.5)
    got = np.stack([vert["red"], vert["green"], vert["blue"]], 1)
    assert np.array_equal(got, want) and tuple(got[0]) == (0, 255, 128)
    # an empty mesh is a valid file
    e = {k: v[:0] for k, v in m.items()}
    vert, faces, _ = parse_ply(mesh.write_ply(str(tmp_path / "empty.ply"), e))
    assert len(vert["x"]) == 0 and faces.shape == (0, 3)


def test_cli_accepts_export_mesh():
    a = trainer.build_parser().parse_args(["export-mesh", "--ckpt", "run", "--out", "m.ply"])
    assert (a.command, a.ckpt, a.out, a.resolution, a.bounds, a.iso, a.mma, a.chunk) == (
        "export-mesh", "run", "m.ply", 256, None, None, "f32", None)
    assert mesh.DEFAULT_BOUNDS == (-1.5,) * 3 + (1.5,) * 3 and mesh.DEFAULT_ISO == 10.0 and mesh.DEFAULT_CHUNK == 1 << 18
    a = trainer.build_parser(run_defaults=False).parse_args(
        ["export-mesh", "--ckpt", "c.ckpt", "--out", "m.ply", "--resolution", "64", "--bounds", "-1", "-2", "-3", "1", "2", "3",
         "--iso", "2.5", "--mma", "bf16x6", "--chunk", "1000"])
    assert (a.resolution, a.bounds, a.iso, a.mma, a.chunk) == (64, [-1.0, -2.0, -3.0, 1.0, 2.0, 3.0], 2.5, "bf16x6", 1000)
    with pytest.raises(SystemExit):
        trainer.build_parser().parse_args(["export-mesh", "--out", "m.ply"])
    sub = [act for act in trainer.build_parser()._actions if hasattr(act, "choices") and act.choices and "export-mesh" in act.choices]
    assert "not measured" in sub[0].choices["export-mesh"].format_help()


def test_grid_frame():
    n, o, s = mesh.grid_frame((-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), 256)
    assert n == (256, 256, 256) and o.dtype == np.float32 and np.array_equal(o, np.float32([-1.5] * 3))
    assert np.array_equal(s, np.float32([3.0 / 255] * 3))
    n, o, s = mesh.grid_frame((0, 0, 0, 1, 2, 3), (3, 5, 7))
    assert n == (3, 5, 7) and np.array_equal(s, np.float32([0.5, 0.5, 0.5]))
    for bad in (1, (4, 4), (4, 1, 4)):
        with pytest.raises(ValueError):
            mesh.grid_frame((0, 0, 0, 1, 1, 1), bad)
    with pytest.raises(ValueError):
        mesh.grid_frame((0, 0, 0, 1, 0, 1), 4)


# ---------------------------------------------------------------------------------------------- the reference itself
def _box(n, lo=-1.0, hi=1.0):
    h = (hi - lo) / (n - 1)
    return (n, n, n), (lo, lo, lo), (h, h, h)


def _closed_report(m):
    return (len(ref.unmatched_edges(m["triangles"])), ref.euler_characteristic(m["triangles"]),
            ref.signed_volume(m["positions"], m["triangles"]))


def test_reference_table_shape():
    assert ref.TRI_COUNT[0] == 0 and ref.TRI_COUNT[255] == 0 and ref.TRI_COUNT.max() == 12
    assert all(ref.TRI_COUNT[p] == ref.TRI_COUNT[255 - p] for p in range(256))
    # a single inside corner 0 or 7 touches all six tetrahedra, any other corner only two of them
    assert ref.TRI_COUNT[1] == 6 and ref.TRI_COUNT[128] == 6 and ref.TRI_COUNT[2] == 2


def test_reference_sphere_is_closed_and_outward():
    shape, o, s = _box(21)
    m = ref.extract(ref.sphere(shape, o, s, (0.03, -0.02, 0.05), 0.8), 0.0, o, s)
    unmatched, euler, volume = _closed_report(m)
    assert (unmatched, euler) == (0, 2) and volume > 0
    assert np.all(np.diff(m["vert_key"]) > 0)  # numbered in ascending (v, dir)
    assert len(np.unique(m["triangles"])) == len(m["vert_key"])  # every vertex is used
    # normals point to lower values: away from the centre
    p = m["positions"][m["triangles"]]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.all(np.einsum("ij,ij->i", nrm, p.mean(1) - np.array([0.03, -0.02, 0.05])) > 0)


def test_reference_two_spheres_and_torus():
    shape, o, s = _box(25)
    two = np.maximum(ref.sphere(shape, o, s, (-0.5, -0.1, 0.0), 0.3), ref.sphere(shape, o, s, (0.45, 0.2, 0.1), 0.35))
    unmatched, euler, volume = _closed_report(ref.extract(two, 0.0, o, s))
    assert (unmatched, euler) == (0, 4) and volume > 0
    unmatched, euler, volume = _closed_report(ref.extract(ref.torus(shape, o, s, (0.02, 0.01, -0.03), 0.55, 0.22), 0.0, o, s))
    assert (unmatched, euler) == (0, 0) and volume > 0
    assert abs(volume / (2 * math.pi ** 2 * 0.55 * 0.22 ** 2) - 1) < 0.05


def test_reference_volume_converges_at_second_order():
    """Sphere volume against (4/3) pi R^3: halving the spacing shrinks the error at least 3x (second order: 4x).  Observed
    ratios here: 4.00 (17 -> 33 vertices per axis) and 4.00 (33 -> 65)."""
    R, c = 0.8, (0.03, -0.02, 0.05)
    errs = []
    for n in (17, 33, 65):
        shape, o, s = _box(n)
        m = ref.extract(ref.sphere(shape, o, s, c, R), 0.0, o, s)
        errs.append(abs(ref.signed_volume(m["positions"], m["triangles"]) - 4.0 / 3.0 * math.pi * R ** 3))
    print("sphere volume errors", errs, "ratios", errs[0] / errs[1], errs[1] / errs[2])
    assert errs[0] / errs[1] >= 3.0 and errs[1] / errs[2] >= 3.0


def test_reference_special_values_and_canonical_form():
    rng = np.random.default_rng(0)
    vol = rng.normal(size=(4, 5, 6)).astype(np.float32)
    vol.ravel()[rng.choice(vol.size, 30, replace=False)] = np.repeat(np.float32([np.nan, np.inf, -np.inf]), 10)
    o, s = (-1.0, 0.5, 2.0), (0.25, 0.5, 1.0)
    m = ref.extract(vol, 0.1, o, s)
    hi = np.array(o) + np.array(s) * (np.array([6, 5, 4]) - 1)
    assert np.all(np.isfinite(m["positions"])) and np.all(m["positions"] >= np.array(o)) and np.all(m["positions"] <= hi)
    canon = ref.canonical(m["triangles"], m["vert_key"])
    perm = rng.permutation(len(m["triangles"]))
    rolled = np.stack([np.roll(t, k) for t, k in zip(m["triangles"][perm], rng.integers(0, 3, len(perm)))])
    assert np.array_equal(ref.canonical(rolled, m["vert_key"]), canon)
    flipped = m["triangles"][:, [0, 2, 1]]
    assert not np.array_equal(ref.canonical(flipped, m["vert_key"]), canon)  # orientation is part of the form
