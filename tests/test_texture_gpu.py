"""GPU checks of the textured mesh export: rsn_texture_points against the numpy restatement of include/rsn.h
(tests/texture_reference.py) by bits -- ragged atlases, partial workgroups, degenerate and out-of-range triangles, sentinels around
the outputs --, bake_textures on an analytic callable, and the route from a checkpoint to OBJ + MTL + four PNG maps on small random
models, by both methods."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, ops, render, texture, trainer
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import texture_reference as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PAD = 1024                      # sentinel words in front of and behind every output
CANARY_I, CANARY_F = -77, -12345.5


def device_points(pos, tri, P, Q=None, n_triangles=None):
    """rsn_texture_points into sentinel-framed buffers -> (face [N,N], point [N,N,3], footprint [N,N]) as numpy; asserts that no
    word outside the N*N rows changed."""
    lib = _abi.load_library()
    T = len(tri) if n_triangles is None else n_triangles
    Q = ref.squares_per_row(T) if Q is None else Q
    N = Q * P
    n = N * N
    pos_t = torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(DEV)
    tri_t = torch.from_numpy(np.ascontiguousarray(tri, dtype=np.int32)).to(DEV)
    face = torch.full((n + 2 * PAD,), CANARY_I, device=DEV, dtype=torch.int32)
    point = torch.full((3 * n + 2 * PAD,), CANARY_F, device=DEV)
    fp = torch.full((n + 2 * PAD,), CANARY_F, device=DEV)
    check(lib.rsn_texture_points(len(pos), ptr(pos_t) if len(pos) else None, T, ptr(tri_t) if len(tri) else None, P, Q,
                                 ptr(face[PAD:]), ptr(point[PAD:]), ptr(fp[PAD:]), ops._stream()))
    torch.cuda.synchronize()
    for buf, canary, m in ((face, CANARY_I, n), (point, CANARY_F, 3 * n), (fp, CANARY_F, n)):
        assert bool((buf[:PAD] == canary).all()) and bool((buf[PAD + m:] == canary).all()), "a word outside the outputs was written"
    return (face[PAD:PAD + n].reshape(N, N).cpu().numpy(), point[PAD:PAD + 3 * n].reshape(N, N, 3).cpu().numpy(),
            fp[PAD:PAD + n].reshape(N, N).cpu().numpy())


def assert_bits(got, want):
    face, point, fp = got
    assert face.shape == want["face"].shape
    assert np.array_equal(face, want["face"])
    assert np.array_equal(point.view(np.int32), want["point"].view(np.int32))
    assert np.array_equal(fp.view(np.int32), want["footprint"].view(np.int32))
    assert np.all(np.isfinite(point)) and np.all(np.isfinite(fp))


@pytest.mark.parametrize("T,P,Q", [(1, 4, None), (2, 5, None), (3, 5, None), (7, 6, None), (129, 4, None), (129, 5, None),
                                   (129, 8, None), (129, 8, 91)])
def test_points_equal_the_reference_by_bits(T, P, Q):
    """T = 1, 3, 7, 129 leave an upper half empty and T = 3, 7, 129 whole squares (Q*Q > S); at T = 129 (Q = 9) N = 36, 45, 72 is no
    multiple of 64 and N*N = 1296, 2025, 5184 texels end in a partial workgroup of 16, 233 and 64 lanes.  Q = 91: N = 728, 529,984
    texels = 2070 tiles of 256 and a quarter -- more than the 2048 workgroups of the largest grid, so the first 23 workgroups walk
    a second tile, the last of them a partial one; what real exports (millions of texels) depend on."""
    pos, tri = ref.triangle_soup(np.random.default_rng(100 * T + P), T)
    want = ref.texture_points(pos, tri, P, Q=Q)
    assert (want["face"] >= 0).any() and (want["face"] < 0).any() and (want["size"] ** 2) % 256 != 0
    assert Q is None or want["size"] ** 2 > 2048 * 256
    assert_bits(device_points(pos, tri, P, Q=Q), want)


def test_shared_vertices_and_a_wider_atlas_than_needed():
    """An indexed mesh (vertices shared between triangles), with Q = 5 where 3 would do: rows of squares without a triangle."""
    rng = np.random.default_rng(7)
    pos = rng.normal(size=(9, 3)).astype(np.float32)
    tri = rng.integers(0, 9, size=(13, 3)).astype(np.int32)
    assert_bits(device_points(pos, tri, 6, Q=5), ref.texture_points(pos, tri, 6, Q=5))


def test_degenerate_triangles_and_mixed_magnitudes():
    rng = np.random.default_rng(8)
    pos = (rng.normal(size=(12, 3)) * np.array([1e-3, 1.0, 1e3])).astype(np.float32)
    tri = np.array([[0, 1, 2], [3, 3, 4], [5, 5, 5], [6, 7, 8], [9, 10, 11], [2, 1, 0]], dtype=np.int32)
    pos[8] = pos[6] + np.float32(0.25) * (pos[7] - pos[6])  # triangle 3: three points of one line, zero area
    want = ref.texture_points(pos, tri, 5)
    assert np.all(want["footprint"][want["face"] == 2] == 0) and (want["face"] == 2).any()
    assert_bits(device_points(pos, tri, 5), want)


def test_a_triangle_with_an_index_out_of_range_is_unused_and_nothing_else_changes():
    pos, tri = ref.triangle_soup(np.random.default_rng(9), 6)
    good = device_points(pos, tri, 5)
    for bad_index in (len(pos), -1, 2 ** 31 - 1, -2 ** 31):
        bad = tri.copy()
        bad[3, 2] = bad_index
        got = device_points(pos, bad, 5)
        assert_bits(got, ref.texture_points(pos, bad, 5))
        gone = good[0] == 3
        assert gone.any() and np.array_equal(got[0], np.where(gone, -1, good[0]))
        assert np.array_equal(got[1].view(np.int32), np.where(gone[..., None], 0, good[1].view(np.int32)))
        assert np.array_equal(got[2].view(np.int32), np.where(gone, 0, good[2].view(np.int32)))
    # without vertices every triangle is out of range
    face, point, fp = device_points(np.zeros((0, 3), np.float32), tri, 5)
    assert np.all(face == -1) and np.all(point == 0) and np.all(fp == 0)


def test_no_triangles_launch_nothing():
    pos, tri = ref.triangle_soup(np.random.default_rng(1), 2)
    face, point, fp = device_points(pos, tri, 4, Q=3, n_triangles=0)
    assert np.all(face == CANARY_I) and np.all(point == CANARY_F) and np.all(fp == CANARY_F)
    at = texture.texture_atlas(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV, dtype=torch.int32), 4)
    assert at["size"] == 4 and at["live"].numel() == 0 and bool((at["face"] == -1).all()) and float(at["point"].abs().max()) == 0.0


def test_texture_atlas_is_the_call_and_two_runs_give_the_same_bits():
    pos, tri = ref.triangle_soup(np.random.default_rng(11), 129)
    pos_t, tri_t = torch.from_numpy(pos).to(DEV), torch.from_numpy(tri).to(DEV)
    a, b = texture.texture_atlas(pos_t, tri_t, 8), texture.texture_atlas(pos_t, tri_t, 8)
    want = ref.texture_points(pos, tri, 8)
    assert (a["size"], a["squares_per_row"], a["texels"]) == (72, 9, 8)
    assert_bits((a["face"].cpu().numpy(), a["point"].cpu().numpy(), a["footprint"].cpu().numpy()), want)
    for k in ("face", "point", "footprint", "live"):
        assert torch.equal(a[k].reshape(-1).view(torch.int32), b[k].reshape(-1).view(torch.int32)), k
    assert np.array_equal(a["live"].cpu().numpy(), np.flatnonzero(want["face"].reshape(-1) >= 0))
    assert np.array_equal(a["uv"], ref.corner_uv(129, 8, 9))
    with pytest.raises(ValueError, match="texels"):
        texture.texture_atlas(pos_t, tri_t, 3)


# ---------------------------------------------------------------------------------------------- baking
def test_bake_an_analytic_callable():
    """The maps hold q(sat(.)) of the callable's values at the reference's points, the stated fill elsewhere, and the linear channel
    reads back within the bound of the CPU test (0.5 / 255 + 1e-5: see test_texture_cpu.test_round_trip_through_a_baked_atlas)."""
    rng = np.random.default_rng(12)
    T, P = 11, 5
    pos, tri = ref.triangle_soup(rng, T)
    c, d = ref.linear_function(pos, rng)
    c32, d32 = torch.tensor(c, dtype=torch.float32, device=DEV), float(np.float32(d))
    calls = []

    def attributes(points, footprint):
        assert points.shape == (footprint.shape[0], 3) and points.device == DEV
        calls.append(int(points.shape[0]))
        x, y, z = points[:, 0], points[:, 1], points[:, 2]
        lin = ((x * c32[0] + y * c32[1]) + z * c32[2]) + d32  # element-wise: the same bits whatever the chunk
        return {"diff": torch.stack([lin, 3.0 * lin - 1.0, 2.0 - 3.0 * lin], dim=1),      # below 0 and above 1 in the gutter
                "tint": torch.stack([footprint, torch.sin(points[:, 0]) * 0.5 + 0.5, points[:, 1] * 0.0 + 0.25], dim=1),
                "roughness": lin, "pred_normals": points / torch.sqrt((x * x + y * y) + z * z)[:, None]}

    at = texture.texture_atlas(torch.from_numpy(pos).to(DEV), torch.from_numpy(tri).to(DEV), P)
    maps = texture.bake_textures(attributes, at, chunk=100)
    torch.cuda.synchronize()
    want = ref.texture_points(pos, tri, P)
    N, live = want["size"], want["face"] >= 0
    n_live = int(live.sum())
    assert sum(calls) == n_live and max(calls) <= 100 and len(calls) == -(-n_live // 100)  # only live texels, in chunks
    assert set(maps) == set(texture.MAPS)
    got = {k: v.cpu().numpy() for k, v in maps.items()}
    for k, v in got.items():
        assert v.shape == (N, N, 3) and v.dtype == np.uint8
        assert np.all(v[~live] == 128), k  # q(0.5) = (int)(127.5 + 0.5), and RSN_VIS_UNIT of (0, 0, 0) is 0.5 too
    # the callable again, on the reference's points (equal to the device's by bits: the tests above)
    vals = attributes(torch.from_numpy(want["point"][live]).to(DEV), torch.from_numpy(want["footprint"][live]).to(DEV))
    vals = {k: v.cpu().numpy() for k, v in vals.items()}
    assert np.array_equal(got["diffuse"][live], ref.quantise(vals["diff"]))
    assert np.array_equal(got["tint"][live], ref.quantise(vals["tint"]))
    assert np.array_equal(got["roughness"][live], np.repeat(ref.quantise(vals["roughness"])[:, None], 3, axis=1))
    half = (vals["pred_normals"] * np.float32(0.5)).astype(np.float32) + np.float32(0.5)
    assert np.array_equal(got["normal"][live], ref.quantise(half))
    assert vals["diff"].min() < 0.0 and vals["diff"].max() > 1.0 and got["diffuse"].min() == 0 and got["diffuse"].max() == 255
    # the round trip through the device-baked roughness map
    err = ref.round_trip_error(got["roughness"][..., 0].astype(np.float64) / 255.0, want["face"], at["uv"], pos, tri, c, d,
                               ref.interior_barycentrics(rng, 2000))
    print(f"round trip of the device-baked map: {err * 255:.4f} / 255")
    assert err <= 0.5 / 255 + 1e-5


# ---------------------------------------------------------------------------------------------- checkpoint -> OBJ
RES, BOUNDS, P_E2E = 12, (-1.2, -1.2, -1.2, 1.2, 1.2, 1.2), 4
SIDE, FOV_DEG, FOG_DEPTH = 16, 40.0, 3.5


def _checkpoint(tmp_path_factory, name, fog):
    """A 4 x 64 field with random weights; fog: the density head a constant sigma = ln 2 / 3.5, so that every ray's median depth is
    about 3.5 and cameras 4 from the origin fuse a surface inside the box (the fixture of the TSDF tests)."""
    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)
    model = trainer.make_model(cfg, seed=3).to(DEV).eval()
    if fog:
        with torch.no_grad():
            model.field.field_output_density.net.weight.zero_()
            model.field.field_output_density.net.bias.fill_(math.log(math.expm1(math.log(2.0) / FOG_DEPTH)) - model.field.density_bias)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    run = tmp_path_factory.mktemp(name) / "run"
    return trainer.save_checkpoint(trainer.checkpoint_path(str(run), 5), model, opt, 5), model


@pytest.fixture(scope="module")
def random_checkpoint(tmp_path_factory):
    return _checkpoint(tmp_path_factory, "random", fog=False)


@pytest.fixture(scope="module")
def fog_checkpoint(tmp_path_factory):
    return _checkpoint(tmp_path_factory, "fog", fog=True)


def two_cameras():
    fx, fy, cx, cy = render.pinhole(SIDE, SIDE, math.radians(FOV_DEG))
    return {"c2w": render.orbit_path(2, (0.0, 0.0, 0.0), 4.0, 20.0), "width": SIDE, "height": SIDE, "fx": fx, "fy": fy, "cx": cx, "cy": cy}


def check_file_set(res, out, surface, model):
    """The six files of an export against the stages by hand: `surface` = the mesh extract_surface (and the filter) return."""
    files = ref.file_set(out)
    blobs = ref.read_all(files)
    assert all(b is not None for b in blobs) and [res["files"][k] for k in ("obj", "mtl", *texture.MAPS)] == files
    o = ref.parse_obj(out)
    pos, tri = surface["positions"].cpu().numpy(), surface["triangles"].cpu().numpy()
    V, T = len(pos), len(tri)
    assert (res["vertices"], res["triangles"]) == (V, T) and T > 0
    assert np.array_equal(o["v"].view(np.int32), pos.view(np.int32)) and np.array_equal(o["fv"], tri) and np.array_equal(o["fvn"], tri)
    Q, N = texture.atlas_shape(T, P_E2E)
    assert (res["texture_size"], res["texels"]) == (N, P_E2E)
    assert np.array_equal(o["fvt"], np.arange(3 * T).reshape(T, 3)) and np.abs(o["vt"] - ref.corner_uv(T, P_E2E, Q).reshape(-1, 2)).max() <= 1e-12
    spacing = res["spacing"]
    field = model.field
    field.set_mma_mode("f32")
    at_v = mesh.vertex_attributes(field, surface["positions"], spacing)
    assert np.array_equal(o["vn"].view(np.int32), at_v["pred_normals"].cpu().numpy().view(np.int32))
    # the maps: the same calls by hand, compared by bits
    want = ref.texture_points(pos, tri, P_E2E)
    live = want["face"] >= 0
    assert res["live_texels"] == int(live.sum()) and res["min_footprint"] == max(spacing) / 8
    attributes = texture.field_attributes(field, spacing)
    vals = attributes(torch.from_numpy(want["point"][live]).to(DEV), torch.from_numpy(want["footprint"][live]).to(DEV))
    vals = {k: v.cpu().numpy() for k, v in vals.items()}
    img = {m: np.asarray(Image.open(f)) for m, f in zip(texture.MAPS, files[2:])}
    for m in texture.MAPS:
        assert img[m].shape == (N, N, 3) and np.all(img[m][~live] == 128), m
    assert np.array_equal(img["diffuse"][live], ref.quantise(vals["diff"])) and np.array_equal(img["tint"][live], ref.quantise(vals["tint"]))
    assert np.array_equal(img["roughness"][live], np.repeat(ref.quantise(vals["roughness"].reshape(-1))[:, None], 3, axis=1))
    half = (vals["pred_normals"] * np.float32(0.5)).astype(np.float32) + np.float32(0.5)
    assert np.array_equal(img["normal"][live], ref.quantise(half))
    assert len(np.unique(img["diffuse"][live])) > 1  # a field, not a constant
    return blobs


def test_export_density_end_to_end(random_checkpoint, tmp_path, capsys):
    ckpt, model = random_checkpoint
    iso = float(mesh.density_grid(model.field, BOUNDS, RES, mma="f32").median())  # a level the random field crosses
    out = str(tmp_path / "a" / "thing.obj")
    res = mesh.export_mesh(ckpt, out, resolution=RES, bounds=BOUNDS, iso=iso, texture=True, texels=P_E2E)
    assert set(res["seconds"]) == {"grid", "count", "emit", "attributes", "atlas", "bake", "write"}
    assert all(t >= 0 for t in res["seconds"].values())
    _, origin, spacing = mesh.grid_frame(BOUNDS, RES)
    surface = mesh.extract_surface(mesh.density_grid(model.field, BOUNDS, RES, mma="f32"), iso, origin, spacing)
    blobs = check_file_set(res, out, surface, model)
    # a second export, through the command line: identical bytes for all six files
    out2 = str(tmp_path / "b" / "thing.obj")
    argv = ["export-mesh", "--ckpt", ckpt, "--out", out2, "--resolution", str(RES), "--iso", repr(iso), "--bounds", *[str(b) for b in BOUNDS],
            "--texture", "--texels", str(P_E2E)]
    assert trainer.main(argv) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    assert f"{res['triangles']} triangles" in line and f"textured with {res['texture_size']} x {res['texture_size']} texels" in line
    assert "atlas" in line and "bake" in line
    assert ref.read_all(ref.file_set(out2)) == blobs
    # without --texture the export is the PLY it was
    ply = mesh.export_mesh(ckpt, str(tmp_path / "m.ply"), resolution=RES, bounds=BOUNDS, iso=iso)
    assert set(ply["seconds"]) == {"grid", "count", "emit", "attributes", "write"} and "texture_size" not in ply
    assert open(tmp_path / "m.ply", "rb").read()[:3] == b"ply"
    # a level nothing reaches: an empty mesh is a valid, empty file set
    empty = mesh.export_mesh(ckpt, str(tmp_path / "e.obj"), resolution=RES, bounds=BOUNDS, iso=3e38, texture=True, texels=P_E2E)
    assert (empty["vertices"], empty["triangles"], empty["texture_size"], empty["live_texels"]) == (0, 0, P_E2E, 0)
    o = ref.parse_obj(str(tmp_path / "e.obj"))
    assert o["v"].shape == (0, 3) and o["fv"].shape == (0, 3) and o["mtllib"] == "e.mtl"
    for f in ref.file_set(str(tmp_path / "e.obj"))[2:]:
        assert np.all(np.asarray(Image.open(f)) == 128) and np.asarray(Image.open(f)).shape == (P_E2E, P_E2E, 3)


def test_export_tsdf_end_to_end(fog_checkpoint, tmp_path):
    ckpt, model = fog_checkpoint
    cams = two_cameras()
    out = str(tmp_path / "a" / "fog.obj")
    res = mesh.export_mesh(ckpt, out, resolution=RES, bounds=BOUNDS, method="tsdf", cameras=cams, texture=True, texels=P_E2E)
    assert set(res["seconds"]) == {"depth", "integrate", "count", "emit", "filter", "attributes", "atlas", "bake", "write"}
    assert res["views"] == 2
    (nx, ny, nz), origin, spacing = mesh.grid_frame(BOUNDS, RES)
    model.field.set_mma_mode("f32")
    tsdf, weight = mesh.fuse_depth(model, cams["c2w"], SIDE, SIDE, cams["fx"], cams["fy"], cams["cx"], cams["cy"], BOUNDS, RES, res["trunc"])
    full = mesh.extract_surface(mesh.tsdf_volume(tsdf, weight, 1.0), 0.0, origin, spacing)
    surface = mesh.drop_unobserved(full, weight, (nx, ny, nz), 1.0)
    blobs = check_file_set(res, out, surface, model)
    out2 = str(tmp_path / "b" / "fog.obj")
    mesh.export_mesh(ckpt, out2, resolution=RES, bounds=BOUNDS, method="tsdf", cameras=cams, texture=True, texels=P_E2E)
    assert ref.read_all(ref.file_set(out2)) == blobs
