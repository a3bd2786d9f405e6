"""CPU-side checks of the textured mesh export: the two properties of the atlas layout of include/rsn.h ("texture atlas") on its numpy
restatement (tests/texture_reference.py), the round trip mesh -> baked atlas -> bilinear lookup, the OBJ / MTL / PNG writer against a
parser written for the tests, the argument errors of the library, the package and the command line -- none of which needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, mesh, texture, trainer
from reflect_sampling_nerf_amd._build import LIB_PATH, build_library
from tests import texture_reference as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -2
U = 2.0 ** -24  # fp32 unit round-off
SIZES = (4, 5, 6, 8)


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


# ---------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("P", SIZES)
def test_no_texel_is_live_for_two_triangles(P):
    """Property (b), from the two live sets as the header words them, each on its own."""
    b, a = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    lower = (a + b <= P - 2) & (a <= P - 3) & (b <= P - 3)
    upper = (a + b >= P - 1) & (a >= 2) & (b >= 2)
    assert not np.any(lower & upper)
    assert np.array_equal(upper, upper.T) and np.array_equal(lower, lower.T)  # symmetric in a <-> b
    up, live = ref.classify(P, a, b)
    assert np.array_equal(live, lower | upper) and np.array_equal(up & live, upper)
    assert P not in (4, 8) or int(live.sum()) == {4: 8, 8: 56}[P]
    # the corners are live texels of their own triangle, and the atlas says so for every triangle of a ragged atlas
    T = 7
    pos, tri = ref.triangle_soup(np.random.default_rng(P), T)
    at = ref.texture_points(pos, tri, P)
    assert at["squares_per_row"] == 2 and at["size"] == 2 * P
    for t in range(T):
        assert int((at["face"] == t).sum()) == int((upper if t % 2 else lower).sum())
    assert int((at["face"] >= 0).sum()) == 4 * int(lower.sum()) + 3 * int(upper.sum())


@pytest.mark.parametrize("P", SIZES)
def test_bilinear_taps_of_interior_points_are_live_texels_of_the_triangle(P):
    """Property (a), on a lattice of 64 steps per side (with its edge and corner points) inside each triangle's corner
    triangle.  The points are combinations with dyadic weights of integer texel centres: exact in float64, so "a weight above zero"
    is meant literally."""
    T, K = 7, 64
    pos, tri = ref.triangle_soup(np.random.default_rng(0), T)
    at = ref.texture_points(pos, tri, P)
    Q, N, face = at["squares_per_row"], at["size"], at["face"]
    i, j = np.meshgrid(np.arange(K + 1), np.arange(K + 1), indexing="ij")
    keep = i + j <= K
    w = np.stack([K - i[keep] - j[keep], i[keep], j[keep]], axis=1) / K  # [n,3]
    for t in range(T):
        q = t // 2
        c = ref.corners(P)[t % 2] + np.array([(q % Q) * P, (q // Q) * P])  # (column, row) of the three corners
        xy = w @ c
        rows, cols, wt = ref.taps_at(xy[:, 0], xy[:, 1], N)
        assert np.all((face[rows, cols] == t) | (wt == 0.0)), f"P={P}: triangle {t} reads a texel that is not its own"


def test_uv_corners_land_on_the_stated_texel_centres():
    for P, T in ((4, 1), (5, 7), (8, 129)):
        Q = ref.squares_per_row(T)
        assert texture.atlas_shape(T, P) == (Q, Q * P)
        uv = texture.atlas_uv(T, P, Q)
        assert uv.shape == (T, 3, 2) and uv.dtype == np.float64 and np.array_equal(uv, ref.corner_uv(T, P, Q))
        N = Q * P
        col, row = uv[..., 0] * N - 0.5, (1.0 - uv[..., 1]) * N - 0.5
        t = np.arange(T)
        want = ref.corners(P)[t % 2] + np.stack([(t // 2 % Q) * P, (t // 2 // Q) * P], axis=1)[:, None, :]
        assert np.abs(col - want[..., 0]).max() < 1e-9 and np.abs(row - want[..., 1]).max() < 1e-9
        # at its corner texels the atlas samples the triangle's own vertices, bit for bit
        pos, tri = ref.triangle_soup(np.random.default_rng(T), T)
        at = ref.texture_points(pos, tri, P)
        assert np.array_equal(at["face"][want[..., 1], want[..., 0]], np.repeat(t[:, None], 3, axis=1))
        assert np.array_equal(at["point"][want[..., 1], want[..., 0]], pos[tri])
    assert texture.atlas_shape(0, 8) == (1, 8) and texture.atlas_uv(0, 8, 1).shape == (0, 3, 2)
    for T in (2, 3, 8, 9, 18, 19, 2 * 2047 * 2047 + 1):
        Q, _ = texture.atlas_shape(T, 4)
        assert 2 * Q * Q >= T and (Q == 1 or 2 * (Q - 1) * (Q - 1) < T)


@pytest.mark.parametrize("P", SIZES + (16,))
def test_round_trip_through_a_baked_atlas(P):
    """A function linear in position, values in [1/3, 2/3] on the mesh, baked into the reference atlas and read back by bilinear
    filtering at random interior points.  Quantised to 8 bits: within 0.5 / 255 + 1e-5 -- a convex combination of values each off
    by at most half a step is off by at most half a step; the 1e-5 covers the fp32 rounding of the sample points.  Unquantised:
    to fp32 rounding.  A sample point is (w0 p0 + u p1) + v p2 with |w0|, u, v <= 1 and |p| <= M: u, v carry one rounding, w0 two
    more, each product and each sum one, the sums of magnitude up to 3 M -- under 16 u M per axis in all, times |c|_1."""
    rng = np.random.default_rng(10 + P)
    T = 5
    pos, tri = ref.triangle_soup(rng, T)
    c, d = ref.linear_function(pos, rng)
    at = ref.texture_points(pos, tri, P)
    live = at["face"] >= 0
    value = at["point"].astype(np.float64) @ c + d
    assert value[live].min() >= -1e-6 and value[live].max() <= 1.0 + 1e-6, "the gutter's extrapolation leaves [0, 1]"
    value = np.where(live, value, 0.5)
    uv = ref.corner_uv(T, P, at["squares_per_row"])
    bary = ref.interior_barycentrics(rng, 2000)
    exact = ref.round_trip_error(value, at["face"], uv, pos, tri, c, d, bary)
    tol = 16.0 * U * float(np.abs(pos).max()) * float(np.abs(c).sum())
    quantised = ref.round_trip_error(ref.quantise(value).astype(np.float64) / 255.0, at["face"], uv, pos, tri, c, d, bary)
    print(f"P={P}: unquantised {exact:.3e} (bound {tol:.3e}); quantised {quantised * 255:.4f} / 255")
    assert exact <= tol
    assert quantised <= 0.5 / 255 + 1e-5


def test_reference_handles_unused_texels():
    rng = np.random.default_rng(2)
    pos, tri = ref.triangle_soup(rng, 4)
    full = ref.texture_points(pos, tri, 5)
    bad = tri.copy()
    bad[2, 1] = len(pos)  # out of range
    at = ref.texture_points(pos, bad, 5)
    gone = full["face"] == 2
    assert gone.any() and np.array_equal(at["face"], np.where(gone, -1, full["face"]))
    assert np.array_equal(at["point"], np.where(gone[..., None], 0, full["point"]))
    assert np.array_equal(at["footprint"], np.where(gone, 0, full["footprint"]))
    unused = at["face"] < 0
    assert np.all(at["point"][unused] == 0) and np.all(at["footprint"][unused] == 0) and np.all(at["footprint"][~unused] > 0)


# ---------------------------------------------------------------------------------------------- OBJ, MTL, PNG
def _random_export(rng, V=11, T=7, P=4):
    Q, N = texture.atlas_shape(T, P)
    m = {"positions": (rng.normal(size=(V, 3)) * np.array([1e-3, 1.0, 1e3])).astype(np.float32),
         "triangles": rng.integers(0, V, size=(T, 3)).astype(np.int32), "pred_normals": rng.normal(size=(V, 3)).astype(np.float32)}
    maps = {name: rng.integers(0, 256, size=(N, N, 3)).astype(np.uint8) for name in texture.MAPS}
    return m, texture.atlas_uv(T, P, Q), maps


def test_obj_round_trip_and_identical_bytes(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(3)
    m, uv, maps = _random_export(rng)
    path = str(tmp_path / "sub" / "thing.obj")
    files = texture.write_obj(path, m, uv, maps)
    assert [files[k] for k in ("obj", "mtl", "diffuse", "tint", "roughness", "normal")] == ref.file_set(path)
    first = ref.read_all(ref.file_set(path))
    assert all(b is not None for b in first) and not [f for f in os.listdir(tmp_path / "sub") if f.endswith(".tmp")]
    o = ref.parse_obj(path)
    assert o["mtllib"] == "thing.mtl" and o["usemtl"] == "thing"
    assert np.array_equal(o["v"], m["positions"]) and np.array_equal(o["vn"], m["pred_normals"])  # %.9g round-trips fp32
    assert np.array_equal(o["fv"], m["triangles"]) and np.array_equal(o["fvn"], m["triangles"])
    assert np.array_equal(o["fvt"], np.arange(21).reshape(7, 3))
    assert o["vt"].shape == (21, 2) and np.abs(o["vt"] - uv.reshape(21, 2)).max() <= 1e-12  # %.12g of values in [0, 1]
    mtl = ref.parse_mtl(files["mtl"])
    assert mtl["newmtl"] == "thing"
    assert (mtl["map_Kd"], mtl["map_Ks"], mtl["map_Pr"], mtl["norm"]) == (
        "thing_diffuse.png", "thing_tint.png", "thing_roughness.png", "thing_normal.png")
    assert any("OBJECT space" in line and "0.5" in line for line in mtl["comments"])
    for name in texture.MAPS:
        img = Image.open(files[name])
        assert img.mode == "RGB" and np.array_equal(np.asarray(img), maps[name])
    texture.write_obj(path, m, uv, maps)
    assert ref.read_all(ref.file_set(path)) == first
    # an empty mesh is a valid file set
    e = {k: v[:0] for k, v in m.items()}
    Q, N = texture.atlas_shape(0, 4)
    grey = {name: np.full((N, N, 3), 128, dtype=np.uint8) for name in texture.MAPS}
    files = texture.write_obj(str(tmp_path / "empty.obj"), e, texture.atlas_uv(0, 4, Q), grey)
    o = ref.parse_obj(files["obj"])
    assert o["v"].shape == (0, 3) and o["fv"].shape == (0, 3) and o["mtllib"] == "empty.mtl"
    assert np.asarray(Image.open(files["normal"])).shape == (4, 4, 3)


# ---------------------------------------------------------------------------------------------- argument errors
def test_package_argument_errors(tmp_path):
    for bad in (3, 0, -8):
        with pytest.raises(ValueError, match="texels"):
            texture.atlas_shape(10, bad)
    assert texture.atlas_shape(2 * 2048 * 2048, 8) == (2048, 16384)
    with pytest.raises(ValueError) as e:
        texture.atlas_shape(2 * 2048 * 2048 + 1, 8)
    assert "--texels" in str(e.value) and "--resolution" in str(e.value) and "16384" in str(e.value)
    with pytest.raises(ValueError, match="16384"):
        texture.atlas_shape(2 * 4096 * 4096 + 1, 4)
    # export_mesh refuses before it reads the checkpoint (which does not exist)
    with pytest.raises(ValueError, match=r"\.obj"):
        mesh.export_mesh(str(tmp_path / "none.ckpt"), str(tmp_path / "m.ply"), texture=True)
    with pytest.raises(ValueError, match="texels"):
        mesh.export_mesh(str(tmp_path / "none.ckpt"), str(tmp_path / "m.obj"), texture=True, texels=3)
    with pytest.raises(ValueError, match=r"\.obj"):
        texture.write_obj(str(tmp_path / "m.ply"), {}, None, {})
    for bad in (0.3, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="min-footprint"):
            texture.field_attributes(None, (0.1, 0.1, 0.2), min_footprint=bad)
    assert texture.footprint_bounds((0.1, 0.1, 0.2)) == pytest.approx((0.2 / 8, 0.2))
    assert texture.footprint_bounds((0.1, 0.1, 0.2), 0.2) == pytest.approx((0.2, 0.2))
    # a footprint above the largest spacing (3 / 63 at 64 vertices per axis) is refused before the checkpoint is read, too
    with pytest.raises(ValueError, match="min-footprint"):
        mesh.export_mesh(str(tmp_path / "none.ckpt"), str(tmp_path / "m.obj"), resolution=64, texture=True, min_footprint=0.05)


def test_cli_flags(capsys):
    base = ["export-mesh", "--ckpt", "run", "--out"]
    a = trainer.build_parser().parse_args(base + ["m.obj", "--texture", "--texels", "6", "--min-footprint", "0.01"])
    assert (a.texture, a.texels, a.min_footprint) == (True, 6, 0.01)
    a = trainer.build_parser().parse_args(base + ["m.ply"])
    assert (a.texture, a.texels, a.min_footprint) == (False, None, None)
    for argv, word in ((base + ["m.ply", "--texels", "8"], "--texels need(s) --texture"),
                       (base + ["m.ply", "--min-footprint", "0.1"], "--min-footprint need(s) --texture"),
                       (base + ["m.ply", "--texture"], "must end in .obj"),
                       (base + ["m.obj", "--texture", "--texels", "3"], "--texels 3"),
                       (base + ["m.obj", "--texture", "--min-footprint", "0"], "--min-footprint 0"),
                       (base + ["m.obj", "--texture", "--resolution", "64", "--min-footprint", "0.05"], "largest grid spacing")):
        with pytest.raises(SystemExit) as e:
            trainer.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    sub = [act for act in trainer.build_parser()._actions if hasattr(act, "choices") and act.choices and "export-mesh" in act.choices]
    text = " ".join(sub[0].choices["export-mesh"].format_help().split())
    assert "--texture" in text and text.count("not measured on a scene") >= 4  # --trunc, --min-weight, --texels, --min-footprint


def test_symbol_is_bound_and_refuses_bad_arguments_before_any_launch(lib):
    """Made-up pointers: a call that reached the device would fault, and there is no device here anyway."""
    assert "rsn_texture_points" in _abi.EXPORTED_SYMBOLS and hasattr(C.CDLL(LIB_PATH), "rsn_texture_points")
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(r"\bint rsn_texture_points\(", header) and re.search(r"#define RSN_ABI_VERSION 18\b", header)
    assert lib.rsn_abi_version() == 18
    p = C.c_void_p(0x1000)

    def call(V=6, pos=p, T=2, tri=p, P=8, Q=1, face=p, point=p, fp=p):
        return lib.rsn_texture_points(V, pos, T, tri, P, Q, face, point, fp, None)

    for kw, word in (({"P": 3}, b"texels=3"), ({"P": 0}, b"texels=0"), ({"P": -4}, b"texels=-4"), ({"Q": 0}, b"squares_per_row=0"),
                     ({"Q": -1}, b"squares_per_row=-1"), ({"T": 3}, b"n_triangles=3"), ({"T": 9, "Q": 2}, b"n_triangles=9"),
                     ({"V": -1}, b"n_vertices=-1"), ({"T": -1}, b"n_triangles=-1"), ({"pos": None}, b"NULL"), ({"tri": None}, b"NULL"),
                     ({"face": None}, b"NULL"), ({"point": None}, b"NULL"), ({"fp": None}, b"NULL")):
        assert call(**kw) == INVALID and word in lib.rsn_last_error(), kw
    assert call(P=4, Q=4097) == UNSUPPORTED and b"16384" in lib.rsn_last_error()
    assert call(P=16385, Q=1) == UNSUPPORTED and call(P=2 ** 30, Q=2 ** 30) == UNSUPPORTED
    assert call(P=3, Q=2 ** 30) == INVALID  # the argument errors come first
    # nothing to launch: no triangles, whatever the pointers; the largest texture is accepted
    assert call(T=0, pos=None, tri=None, face=None, point=None, fp=None) == OK
    assert call(T=0, P=4, Q=4096, pos=None, tri=None, face=None, point=None, fp=None) == OK
    assert call(T=0, V=0, P=16384, Q=1) == OK
