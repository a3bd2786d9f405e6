"""GPU checks of the mesh export: rsn_mesh_count / rsn_mesh_emit against the numpy restatement of include/rsn.h
(tests/mesh_reference.py) -- every pattern of one cell, ragged grids, a volume whose block sums need several passes of the
second scan level, closed and open surfaces, empty volumes, truncated capacities, special values -- and the route from a
checkpoint to a PLY file on a small random model."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, ops, trainer
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import mesh_reference as ref
from tests.mesh_reference import parse_ply

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SCAN_SPAN = 1024  # grid vertices per workgroup (first scan level) = block sums per pass of the second level's one workgroup
U = 2.0 ** -24    # fp32 unit round-off


def position_tolerance(shape_xyz, origin, spacing):
    """Bound on |device position - fp64 reference| per coordinate, to first order in u = 2^-24, every device step being one
    correctly rounded fp32 operation.  M = the largest |coordinate| of a grid vertex, h = the largest spacing.
      p_lo = fl(o + fl(s i)): |s i| = |p_lo - o| <= 2 M, so 2 M u from the product and M u from the sum: 3 M u; p_hi alike.
      With t in [0, 1], p = (1 - t) p_lo + t p_hi is a convex combination: the end points' errors contribute at most 3 M u.
      t = fl(fl(iso - f_lo) / fl(f_hi - f_lo)): three roundings, relative 3 u (the inputs are exact fp32 values);
      d = fl(p_hi - p_lo): u; fl(t d): u; together 5 u |t d| <= 5 h u.  The final sum rounds once more: M u.
    Total (4 M + 5 h) u; asserted with 6 h, the extra h u covering the second-order terms.  Since h <= 2 M on any grid this
    is at most 16 M u = 2^-20 M, the bound the contract started from, and about 4x tighter on a grid of many cells."""
    n = np.asarray(shape_xyz, dtype=np.float64)
    o, s = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    M = float(np.max(np.maximum(np.abs(o), np.abs(o + s * (n - 1)))))
    tol = (4.0 * M + 6.0 * float(s.max())) * U
    assert tol <= 2.0 ** -20 * M
    return tol


def _f3(x):
    return (C.c_float * 3)(*[float(v) for v in x])


def device_count(vol_t, iso):
    """-> (workspace tensor, counts tensor [2] on the device)."""
    lib = _abi.load_library()
    nz, ny, nx = vol_t.shape
    nbytes = int(lib.rsn_mesh_workspace_bytes(nx, ny, nz))
    assert nbytes > 0
    ws = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
    cnt = torch.full((2,), -7, device=DEV, dtype=torch.int32)
    check(lib.rsn_mesh_count(nx, ny, nz, ptr(vol_t), float(iso), ptr(ws), nbytes, ptr(cnt), ops._stream()))
    return ws, cnt


def device_extract(vol, iso, origin, spacing):
    """The public route, as numpy: positions [V,3] fp32, triangles [T,3], vert_key [V]."""
    vol_t = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV)
    m = mesh.extract_surface(vol_t, iso, origin, spacing)
    torch.cuda.synchronize()
    assert m["positions"].dtype == torch.float32 and m["triangles"].dtype == torch.int32 and m["vert_key"].dtype == torch.int32
    return {k: v.cpu().numpy() for k, v in m.items()}


def assert_same_mesh(got, want, tol=None):
    """Canonically equal, and -- the reference emits in the header's order -- equal entry by entry as well."""
    assert got["vert_key"].shape == want["vert_key"].shape and got["triangles"].shape == want["triangles"].shape
    assert np.array_equal(got["vert_key"], want["vert_key"])  # numbered in ascending (v, dir)
    assert np.array_equal(ref.canonical(got["triangles"], got["vert_key"]), ref.canonical(want["triangles"], want["vert_key"]))
    assert np.array_equal(got["triangles"], want["triangles"])  # cell, permutation and in-tetrahedron order
    if tol is not None and len(want["positions"]):
        err = float(np.abs(got["positions"].astype(np.float64) - want["positions"]).max())
        print(f"position error {err:.3e} (bound {tol:.3e})")
        assert err <= tol


def test_all_256_patterns_of_one_cell():
    rng = np.random.default_rng(1)
    o, s = (0.25, -1.0, 3.0), (0.5, 1.25, 0.75)
    tol = position_tolerance((2, 2, 2), o, s)
    for pattern in range(256):
        mag = rng.uniform(0.1, 2.0, size=8)
        vol = np.array([mag[L] if (pattern >> L) & 1 else -mag[L] for L in range(8)], dtype=np.float32).reshape(2, 2, 2)
        want = ref.extract(vol, 0.0, o, s)
        assert len(want["triangles"]) == ref.TRI_COUNT[pattern]
        assert_same_mesh(device_extract(vol, 0.0, o, s), want, tol)


@pytest.mark.parametrize("shape_xyz", [(5, 7, 3), (19, 23, 17)])
def test_ragged_gyroid(shape_xyz):
    """No dimension is a multiple of anything; 19 x 23 x 17 = 7429 vertices span 8 workgroups, the last one partial."""
    o, s = (-3.1, -2.7, -1.9), (0.37, 0.41, 0.29)
    vol = ref.gyroid(shape_xyz, o, s)
    want = ref.extract(vol, 0.05, o, s)
    assert len(want["triangles"]) > 0
    assert_same_mesh(device_extract(vol, 0.05, o, s), want, position_tolerance(shape_xyz, o, s))


def test_large_scan_counts_closed_and_bit_identical():
    """161^3 = 4,173,281 vertices = 4,076 workgroups of SCAN_SPAN: the second level's one workgroup takes 4 passes of SCAN_SPAN
    block sums, carrying between them.  The volume is sin x sin y sin z - 1/2 on [0, 4 pi]^3: 32 closed blobs, one in every
    other octant of the 4 x 4 x 4 half-period cells, none touching the boundary (where the product is 0)."""
    n = 161
    assert n ** 3 > SCAN_SPAN * SCAN_SPAN * 3
    h = np.float32(4.0 * math.pi / (n - 1))
    o, s = (0.0, 0.0, 0.0), (h, h, h)
    x, y, z = ref.grid_points((n, n, n), o, s)
    vol = (np.sin(x) * np.sin(y) * np.sin(z) - 0.5).astype(np.float32)
    want_v, want_t = ref.counts(vol, 0.0)
    vol_t = torch.from_numpy(vol).to(DEV)
    a = mesh.extract_surface(vol_t, 0.0, o, s)
    b = mesh.extract_surface(vol_t, 0.0, o, s)
    torch.cuda.synchronize()
    assert (a["positions"].shape[0], a["triangles"].shape[0]) == (want_v, want_t) and want_t > 100000
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    tri, key = a["triangles"].cpu().numpy(), a["vert_key"].cpu().numpy()
    assert np.all(np.diff(key.astype(np.int64)) > 0)
    assert tri.min() == 0 and tri.max() == want_v - 1
    assert len(ref.unmatched_edges(tri)) == 0
    assert ref.euler_characteristic(tri) == 2 * 32
    assert ref.signed_volume(a["positions"].cpu().numpy(), tri) > 0


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_closed_surfaces(name):
    n = 25
    h = 2.0 / (n - 1)
    shape, o, s = (n, n, n), (-1.0, -1.0, -1.0), (h, h, h)
    if name == "sphere":
        vol, euler = ref.sphere(shape, o, s, (0.03, -0.02, 0.05), 0.8), 2
    else:
        vol, euler = ref.torus(shape, o, s, (0.02, 0.01, -0.03), 0.55, 0.22), 0
    got, want = device_extract(vol, 0.0, o, s), ref.extract(vol, 0.0, o, s)
    assert len(ref.unmatched_edges(got["triangles"])) == 0
    assert ref.euler_characteristic(got["triangles"]) == euler
    v_got, v_want = ref.signed_volume(got["positions"], got["triangles"]), ref.signed_volume(want["positions"], want["triangles"])
    print(f"{name}: volume {v_got:.9f}, reference mesh {v_want:.9f}")
    assert v_got > 0 and abs(v_got / v_want - 1.0) <= 1e-5


def test_open_surface_is_open_only_on_the_boundary():
    """A sphere that leaves the box through its y and z faces: each edge without a partner lies in a boundary face."""
    shape, o, s = (13, 11, 9), (-1.0, -0.8, -0.6), (np.float32(1 / 6), np.float32(0.16), np.float32(0.15))
    vol = ref.sphere(shape, o, s, (0.05, 0.02, -0.01), 0.9)
    got = device_extract(vol, 0.0, o, s)
    assert_same_mesh(got, ref.extract(vol, 0.0, o, s), position_tolerance(shape, o, s))
    open_edges = ref.unmatched_edges(got["triangles"])
    assert len(open_edges) > 0
    lo = np.float32(o)
    hi = lo + np.float32(s) * (np.float32(shape) - np.float32(1.0))  # the device's own fp32 arithmetic
    pa, pb = got["positions"][open_edges[:, 0]], got["positions"][open_edges[:, 1]]
    on_face = ((pa == lo) & (pb == lo)) | ((pa == hi) & (pb == hi))
    assert np.all(on_face.any(axis=1))


def test_empty_volumes_and_zero_capacity():
    lib = _abi.load_library()
    nx, ny, nz = 9, 6, 5
    for value in (1.0, -1.0, float("nan")):
        vol_t = torch.full((nz, ny, nx), value, device=DEV)
        ws, cnt = device_count(vol_t, 0.0)
        assert cnt.tolist() == [0, 0]
        assert lib.rsn_mesh_emit(nx, ny, nz, ptr(vol_t), 0.0, _f3((0, 0, 0)), _f3((1, 1, 1)), ptr(ws), ws.numel(), 0, 0, None,
                                 None, None, ops._stream()) == 0
        m = mesh.extract_surface(vol_t, 0.0, (0, 0, 0), (1, 1, 1))
        assert m["positions"].shape == (0, 3) and m["triangles"].shape == (0, 3) and m["vert_key"].shape == (0,)
    # zero capacity on a volume that has a surface
    vol_t = torch.from_numpy(ref.gyroid((nx, ny, nz), (0, 0, 0), (0.7, 0.7, 0.7))).to(DEV)
    ws, cnt = device_count(vol_t, 0.0)
    assert min(cnt.tolist()) > 0
    assert lib.rsn_mesh_emit(nx, ny, nz, ptr(vol_t), 0.0, _f3((0, 0, 0)), _f3((1, 1, 1)), ptr(ws), ws.numel(), 0, 0, None, None,
                             None, ops._stream()) == 0
    torch.cuda.synchronize()


def test_truncated_capacities_write_a_prefix_and_nothing_else():
    lib = _abi.load_library()
    shape_xyz, o, s = (19, 23, 17), (-3.1, -2.7, -1.9), (0.37, 0.41, 0.29)
    nx, ny, nz = shape_xyz
    vol_t = torch.from_numpy(ref.gyroid(shape_xyz, o, s)).to(DEV)
    full = mesh.extract_surface(vol_t, 0.05, o, s)
    V, T = full["positions"].shape[0], full["triangles"].shape[0]
    ws, cnt = device_count(vol_t, 0.05)
    assert cnt.tolist() == [V, T]
    CANARY_F, CANARY_I, PAD = -12345.5, -77, 4096
    for mv, mt in ((V // 2 + 1, T // 3 + 1), (1, 1), (V - 1, T - 1), (V, 0), (0, T)):
        pos = torch.full(((mv + PAD) * 3,), CANARY_F, device=DEV)
        key = torch.full((mv + PAD,), CANARY_I, device=DEV, dtype=torch.int32)
        tri = torch.full(((mt + PAD) * 3,), CANARY_I, device=DEV, dtype=torch.int32)
        check(lib.rsn_mesh_emit(nx, ny, nz, ptr(vol_t), 0.05, _f3(o), _f3(s), ptr(ws), ws.numel(), mv, mt, ptr(pos), ptr(key),
                                ptr(tri), ops._stream()))
        torch.cuda.synchronize()
        assert torch.equal(pos[: mv * 3].view(torch.int32), full["positions"].reshape(-1)[: mv * 3].view(torch.int32))
        assert torch.equal(key[:mv], full["vert_key"][:mv]) and torch.equal(tri[: mt * 3], full["triangles"].reshape(-1)[: mt * 3])
        assert bool((pos[mv * 3:] == CANARY_F).all()) and bool((key[mv:] == CANARY_I).all()) and bool((tri[mt * 3:] == CANARY_I).all())


def test_special_values_give_finite_positions_inside_the_box():
    rng = np.random.default_rng(5)
    shape_xyz, o, s = (11, 9, 7), (-2.0, 0.5, 10.0), (0.3, 0.45, 0.2)
    vol = rng.normal(size=shape_xyz[::-1]).astype(np.float32)
    special = np.float32([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-42, -0.0])
    vol.ravel()[rng.choice(vol.size, 40 * len(special), replace=False)] = np.repeat(special, 40)
    lo = np.float32(o)
    hi = lo + np.float32(s) * (np.float32(shape_xyz) - np.float32(1.0))
    for iso in (0.1, 0.0, float("inf"), -float("inf"), 3e38, float("nan")):
        got = device_extract(vol, iso, o, s)
        want_v, want_t = ref.counts(vol, iso)
        assert (len(got["positions"]), len(got["triangles"])) == (want_v, want_t)
        assert np.all(np.isfinite(got["positions"])) and np.all(got["positions"] >= lo) and np.all(got["positions"] <= hi)
        want = ref.extract(vol, iso, o, s)
        assert np.array_equal(got["vert_key"], want["vert_key"]) and np.array_equal(got["triangles"], want["triangles"])
    assert ref.counts(vol, 0.1)[0] > 0 and ref.counts(vol, float("nan")) == (0, 0)


# ---------------------------------------------------------------------------------------------- checkpoint -> PLY
@pytest.fixture(scope="module")
def small_model():
    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)
    model = trainer.make_model(cfg, seed=3).to(DEV).eval()
    return cfg, model


RES, BOUNDS = 20, (-1.2, -1.2, -1.2, 1.2, 1.2, 1.2)  # both sides of the contraction (|x| = 1) are in play


def test_density_grid_is_the_fields_density(small_model):
    _, model = small_model
    field = model.field
    vol = mesh.density_grid(field, BOUNDS, RES, mma="f32")
    assert vol.shape == (RES, RES, RES) and vol.dtype == torch.float32 and bool(torch.isfinite(vol).all())
    assert torch.equal(mesh.density_grid(field, BOUNDS, RES, chunk=1000), vol)
    assert torch.equal(mesh.density_grid(field, BOUNDS, (RES, RES, RES)), vol)
    _, origin, spacing = mesh.grid_frame(BOUNDS, RES)
    g = torch.Generator().manual_seed(0)
    v = torch.randint(0, RES ** 3, (200,), generator=g)
    ijk = torch.stack([v % RES, (v // RES) % RES, v // (RES * RES)], dim=1).to(torch.float32).to(DEV)
    o, s = torch.from_numpy(origin).to(DEV), torch.from_numpy(spacing).to(DEV)
    mean = o + s * ijk
    assert bool((mean.norm(dim=-1) > 1).any()) and bool((mean.norm(dim=-1) < 1).any())
    cov = torch.diag_embed((s * s / 12.0).expand(200, 3))
    m, c = field.contract(mean, cov)
    sigma, _ = field.get_density(m, c)
    assert torch.equal(sigma.reshape(-1), vol.reshape(-1)[v.to(DEV)])


def test_export_mesh_through_the_cli(small_model, tmp_path, capsys):
    cfg, model = small_model
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    ckpt = trainer.save_checkpoint(trainer.checkpoint_path(str(tmp_path / "run"), 7), model, opt, 7)
    iso = float(mesh.density_grid(model.field, BOUNDS, RES, mma="f32").median())
    out = str(tmp_path / "cli.ply")
    argv = ["export-mesh", "--ckpt", str(tmp_path / "run"), "--out", out, "--resolution", str(RES), "--iso", repr(iso),
            "--bounds", *[str(b) for b in BOUNDS]]
    assert trainer.main(argv) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    res = mesh.export_mesh(ckpt, str(tmp_path / "direct.ply"), resolution=RES, bounds=BOUNDS, iso=iso)
    assert res["vertices"] > 0 and res["triangles"] > 0 and res["step"] == 7 and res["iso"] == iso
    assert f"{res['vertices']} vertices, {res['triangles']} triangles" in line
    assert set(res["seconds"]) == {"grid", "count", "emit", "attributes", "write"} and all(t >= 0 for t in res["seconds"].values())
    assert open(out, "rb").read() == open(res["out"], "rb").read()  # the export is deterministic
    vert, faces, _ = parse_ply(out)
    assert len(vert["x"]) == res["vertices"] and faces.shape == (res["triangles"], 3)
    assert faces.min() == 0 and faces.max() == res["vertices"] - 1
    pos = np.stack([vert["x"], vert["y"], vert["z"]], 1)
    assert np.all(np.isfinite(pos)) and np.all(np.abs(pos) <= np.float32(1.2) * (1 + 2 ** -22))
    nrm = np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(nrm, axis=1) - 1.0) < 1e-5)
    for k in ("roughness", "tint_r", "tint_g", "tint_b"):
        assert np.all(np.isfinite(vert[k])) and np.all(vert[k] >= 0.0) and np.all(vert[k] <= 1.0)
    # the colour bytes are the quantised diffuse colour of the field at the vertices
    at = mesh.vertex_attributes(model.field, torch.from_numpy(pos).to(DEV), res["spacing"])
    want = np.floor(np.clip(at["diff"].cpu().numpy(), 0, 1) * 255 + 0.5).astype(np.uint8)
    assert np.array_equal(np.stack([vert["red"], vert["green"], vert["blue"]], 1), want)
    assert np.array_equal(at["roughness"].cpu().numpy(), vert["roughness"])
