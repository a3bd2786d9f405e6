"""CPU checks of the decimation: the numpy restatement of include/rsn.h (tests/decimate_reference.py) has the properties the rule
was chosen for -- balanced directed edges on closed inputs, fins cancelled, vertices inside their cells --, its group rule and its
cell assignment give the stated answers on constructed inputs, the face-budget search ends where it says, and the plumbing (header,
binding, library, argument errors, command line) is in place.  The device is held to the restatement in tests/test_decimate_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from reflect_sampling_nerf_amd import _abi, decimate, mesh, trainer
from reflect_sampling_nerf_amd._build import LIB_PATH, build_library
from tests import decimate_reference as ref
from tests import mesh_reference as mref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = ref.BOX
CELLS = (3, 5, 6, 8, 12, 16)
closed_mesh = ref.fixture_mesh


def run(name, n):
    pos, tri = closed_mesh(name)
    dims, origin, cell = ref.cell_frame(BOUNDS, n)
    return ref.decimate(pos, tri, origin, cell, dims), (dims, origin, cell)


@pytest.mark.parametrize("name", ["sphere_24", "sphere_33", "torus_33"])
def test_closed_inputs_stay_balanced(name):
    cancelled = {}
    for n in CELLS:
        d, _ = run(name, n)
        V, T, degenerate, pairs = d["counts"]
        cancelled[n] = pairs
        assert T + degenerate + 2 * pairs == len(closed_mesh(name)[1])
        assert len(np.unique(d["triangles"])) == V and (T == 0 or d["triangles"].min() == 0)  # every vertex is used
        # (the torus lies inside one layer of three cells per axis: a closed surface mapped into a plane cancels completely)
        assert T > 0 or (name, n) == ("torus_33", 3)
        assert ref.edge_imbalance(d["triangles"]) == 0, n
        if name.startswith("sphere"):
            assert len(mref.unmatched_edges(d["triangles"])) == 0 and mref.euler_characteristic(d["triangles"]) == 2, n
    print(name, "cancelled pairs per n:", cancelled)
    assert cancelled[5] > 0  # fins exist and cancel: without them the rule is untested


@pytest.mark.parametrize("name", ["sphere_33", "torus_33"])
def test_vertices_stay_inside_their_cells(name):
    """The representative is a mean of points of the cell's closed box, so it lies in the box -- up to the one rounding to fp32 of the
    result (half an ulp of the largest coordinate, 2^-24 relative to the box) and the fp32 rounding of the cell's own corners
    o + c i against which it is compared here in fp64: 2^-22 covers both.  It is therefore within the cell's diagonal of every
    input vertex that mapped to it."""
    pos, tri = closed_mesh(name)
    for n in (5, 12):
        d, (dims, origin, cell) = run(name, n)
        o, c = origin.astype(np.float64), cell.astype(np.float64)
        cells = d["cells"]
        ijk = np.stack([cells % n, (cells // n) % n, cells // (n * n)], axis=1).astype(np.float64)
        p = d["positions"].astype(np.float64)
        slack = 2.0 ** -22
        assert np.all(p >= o + c * ijk - slack) and np.all(p <= o + c * (ijk + 1.0) + slack)
        flat, _, _ = ref.vertex_cells(pos, origin, cell, dims)
        at = np.searchsorted(cells, flat)
        mine = (at < len(cells)) & (cells[np.minimum(at, len(cells) - 1)] == flat)
        dist = np.linalg.norm(pos[mine].astype(np.float64) - p[at[mine]], axis=1)
        assert dist.max() <= np.linalg.norm(c) * (1 + 1e-6)


# ---- constructed groups: four cells along x, two along y and z; cell (i, j, k) has the centre below
DIMS, ORIGIN, CELL = (4, 2, 2), np.zeros(3, np.float32), np.ones(3, np.float32)


def centre(i, j, k, shift=0.0):
    return [i + 0.5 + shift, j + 0.5, k + 0.5]


def constructed(copies):
    """Triangles over the cells A = (0,0,0) < B = (1,0,0) < C = (0,1,0) in flat id: `copies` is a string of '+' and '-'; every copy
    has its own three vertices.  -> (positions, triangles)."""
    pos, tri = [], []
    for n, s in enumerate(copies):
        a, b, c = centre(0, 0, 0, 0.01 * n), centre(1, 0, 0, 0.01 * n), centre(0, 1, 0, 0.01 * n)
        pos += [b, c, a] if s == "+" else [c, b, a]  # a rotation of (A, B, C), or of (A, C, B)
        tri.append([3 * n, 3 * n + 1, 3 * n + 2])
    return np.asarray(pos, np.float32), np.asarray(tri, np.int64)


def test_constructed_groups():
    pos, tri = constructed("++-")  # two + and one -: one + survives, the lowest index
    d = ref.decimate(pos, tri, ORIGIN, CELL, DIMS)
    assert d["counts"] == (3, 1, 0, 1)
    # triangle 0 with its corners in its own order (B, C, A) -> new ids of the cells 1, 4, 0 in ascending cell order: 1, 2, 0
    assert d["triangles"].tolist() == [[1, 2, 0]] and d["cells"].tolist() == [0, 1, 4]
    pos, tri = constructed("-++")
    assert ref.decimate(pos, tri, ORIGIN, CELL, DIMS)["triangles"].tolist() == [[1, 2, 0]]  # triangle 1 is the first +
    keep, _, _ = ref.resolve(tri, ref.vertex_cells(pos, ORIGIN, CELL, DIMS)[0], len(pos))
    assert keep.tolist() == [False, True, False]
    pos, tri = constructed("++")  # multiplicity is kept
    d = ref.decimate(pos, tri, ORIGIN, CELL, DIMS)
    assert d["counts"] == (3, 2, 0, 0) and d["triangles"].tolist() == [[1, 2, 0], [1, 2, 0]]
    # the representative of cell A is the fixed-point mean of its two vertices, x = 0.5 and 0.51 (as fp32), rounded once
    q = [int(np.rint(np.float32(x) * np.float32(2 ** 20))) for x in (0.5, 0.51)]
    assert q == [524288, 534774] and d["positions"][0].tolist() == [float(np.float32(sum(q) / 2 * 2.0 ** -20)), 0.5, 0.5]
    pos, tri = constructed("+-")  # a flat fin: nothing survives and its vertices vanish
    d = ref.decimate(pos, tri, ORIGIN, CELL, DIMS)
    assert d["counts"] == (0, 0, 0, 1) and d["positions"].shape == (0, 3) and d["triangles"].shape == (0, 3)
    pos, tri = constructed("+")
    for bad in ([0, 1, 3], [-1, 1, 2], [0, 2 ** 31 - 1, 2]):  # an index outside [0, V) counts as degenerate
        d = ref.decimate(pos, np.asarray([bad, [0, 1, 2]], np.int64), ORIGIN, CELL, DIMS)
        assert d["counts"] == (3, 1, 1, 0)
    d = ref.decimate(pos, np.asarray([[0, 0, 1], [0, 1, 2]], np.int64), ORIGIN, CELL, DIMS)  # two corners in one cell
    assert d["counts"] == (3, 1, 1, 0)


SPECIAL = np.asarray([1.0, 2.0, 0.999999940395, 4.0, 4.5, -0.25, 1e30, -1e30, np.nan, np.inf, -np.inf, 3.9999998, 0.0, -0.0, 2.5],
                     dtype=np.float32)
SPECIAL_CELL = [1, 2, 0, 3, 3, 0, 3, 0, 0, 0, 0, 3, 0, 0, 2]
SPECIAL_Q = [0, 0, 1 << 20, 1 << 20, 1 << 20, 0, 1 << 20, 0, 0, 0, 0, 1048576, 0, 0, 1 << 19]


def test_cell_assignment_edges():
    """By value, on an axis of four unit cells from 0: a coordinate exactly on an interior face belongs to the upper cell; the upper
    box face and everything outside to the nearest boundary cell (at its far or near face: q = 2^20 or 0); NaN and the infinities
    become u = 0."""
    i, q = ref.axis_cells(SPECIAL, 0.0, 1.0, 4)
    assert i.tolist() == SPECIAL_CELL
    assert q.tolist() == SPECIAL_Q
    # a frame with a rounded quotient: u = (p - o) / c in fp32, step by step
    p, o, c = np.float32(0.7), np.float32(-1.2), np.float32(0.3)
    u = np.float32(np.float32(p - o) / c)
    i, q = ref.axis_cells(np.asarray([p]), o, c, 8)
    assert i[0] == int(np.floor(u)) == 6 and q[0] == int(np.rint(np.float32(np.float32(u - np.float32(6.0)) * np.float32(2 ** 20))))
    # a grid past 2^24 cells on an axis: the clamp is on integers
    i, _ = ref.axis_cells(np.asarray([3e8, 16777217.0], np.float32), 0.0, 1.0, (1 << 27))
    assert i.tolist() == [(1 << 27) - 1, 16777216]


def test_search_on_the_sphere():
    pos, tri = closed_mesh("sphere_24")
    max_cells = 23
    counts = {n: ref.survivors(pos, tri, BOUNDS, n) for n in range(2, max_cells + 1)}
    print("survivors per n:", counts)
    for target in (1, 8, 50, 200, 1000, 3000, 5000, 10 ** 6):
        d, st = ref.decimate_to(pos, tri, BOUNDS, target, max_cells)
        n = st["n"]
        assert st["probes"] and all(counts[k] == c for k, c in st["probes"]) and len(st["probes"]) <= 2 + 5
        assert decimate.search_cells(counts.__getitem__, target, max_cells) == (n, st["probes"], st["over_budget"])
        if st["over_budget"]:
            assert n == 2 and counts[2] > target
            continue
        assert d["counts"][1] == counts[n] <= target
        assert n == max_cells or counts[n + 1] > target
    assert ref.decimate_to(pos, tri, BOUNDS, 1, max_cells)[1]["over_budget"]


def test_search_when_the_count_is_not_monotone():
    """The count of a real input that is not monotone in n: four copies of a small triangle around the centre of the box straddle
    three cells for every even n and sit inside one cell for every odd n."""
    e = 0.01
    one = [[e, -e, -e], [-e, e, -e], [-e, -e, e]]
    pos = np.asarray(one * 4, np.float32)
    tri = np.arange(12, dtype=np.int64).reshape(4, 3)
    counts = {n: ref.survivors(pos, tri, BOUNDS, n) for n in range(2, 10)}
    assert [counts[n] for n in range(2, 10)] == [4, 0, 4, 0, 4, 0, 4, 0]
    for search in (ref.search_cells, decimate.search_cells):
        assert search(counts.__getitem__, 2, 9)[::2] == (9, False)  # the finest grid fits: taken
        n, probes, over = search(counts.__getitem__, 2, 8)  # neither end fits: two cells per axis, and it says so
        assert (n, over, [p[0] for p in probes]) == (2, True, [8, 2])
    # a made-up count with dips: the search keeps a lower end that fits, so it ends on an n that fits whose successor does not,
    # and the guard walk behind it never has to step
    table = {2: 10, 3: 50, 4: 30, 5: 80, 6: 20, 7: 90, 8: 95, 9: 40, 10: 99, 11: 120}
    for search in (ref.search_cells, decimate.search_cells):
        for target in range(10, 121, 5):
            n, probes, over = search(table.__getitem__, target, 11)
            assert not over and table[n] <= target and (n == 11 or table[n + 1] > target)
            assert (n, table[n]) in probes  # a probed n: the walk did not move
        assert search(table.__getitem__, 9, 11)[::2] == (2, True)
        assert search(lambda n: None if n > 6 else table[n], 60, 11)[0] == 6  # an n that cannot be run counts as too many


def test_search_argument_errors():
    with pytest.raises(ValueError):
        decimate.search_cells(lambda n: 0, 0, 8)
    with pytest.raises(ValueError):
        decimate.search_cells(lambda n: 0, 10, 1)


# ---------------------------------------------------------------------------------------------------------------- plumbing
NEW_SYMBOLS = ("rsn_decimate_workspace_bytes", "rsn_decimate_cluster", "rsn_decimate_resolve", "rsn_decimate_count", "rsn_decimate_emit")


@pytest.fixture(scope="module")
def lib():
    build_library()
    return _abi.load_library()


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    assert re.search(r"#define RSN_ABI_VERSION 18\b", header) and lib.rsn_abi_version() == 18 == _abi.RSN_ABI_VERSION
    raw = C.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(raw, name), name


def test_argument_errors_come_before_any_launch(lib):
    """Made-up pointers: a call that reached the device would fault, and there is no device here anyway (a launch would answer
    RSN_ERR_HIP, not RSN_ERR_INVALID_ARGUMENT)."""
    p = C.c_void_p(0x1000)
    good_o, good_c = _abi.float3((0, 0, 0)), _abi.float3((1, 1, 1))
    big = 1 << 30

    def cluster(V=6, pos=p, T=2, tri=p, o=good_o, c=good_c, n=(4, 4, 4), ws=p, nbytes=big, keys=p, counts=p):
        return lib.rsn_decimate_cluster(V, pos, T, tri, o, c, *n, ws, nbytes, keys, counts, None)

    def emit(V=6, pos=p, T=2, tri=p, o=good_o, c=good_c, n=(4, 4, 4), ws=p, nbytes=big, mv=1, mt=1, op=p, ot=p):
        return lib.rsn_decimate_emit(V, pos, T, tri, o, c, *n, ws, nbytes, mv, mt, op, ot, None)

    nan, inf = float("nan"), float("inf")
    for call in (cluster, emit):
        for kw, word in (({"n": (0, 4, 4)}, b"0 x 4 x 4 cells"), ({"n": (4, 4, -1)}, b"4 x 4 x -1 cells"), ({"V": -1}, b"n_vertices=-1"),
                         ({"T": -3}, b"n_triangles=-3"), ({"o": _abi.float3((0, nan, 0))}, b"axis 1"),
                         ({"o": _abi.float3((inf, 0, 0))}, b"axis 0"), ({"c": _abi.float3((1, 1, 0))}, b"axis 2"),
                         ({"c": _abi.float3((1, -1, 1))}, b"axis 1"), ({"c": _abi.float3((nan, 1, 1))}, b"axis 0"),
                         ({"c": _abi.float3((1, inf, 1))}, b"axis 1"), ({"pos": None}, b"NULL"), ({"tri": None}, b"NULL"),
                         ({"ws": None}, b"workspace is NULL"), ({"o": None}, b"origin3 or cell3 is NULL"),
                         ({"ws": C.c_void_p(0x1004)}, b"8-byte aligned")):
            assert call(**kw) == -1 and word in lib.rsn_last_error(), (call.__name__, kw, lib.rsn_last_error())
    assert cluster(keys=None) == -1 and cluster(counts=None) == -1
    assert emit(mv=-1) == -1 and b"max_vertices=-1" in lib.rsn_last_error()
    assert emit(op=None) == -1 and emit(ot=None) == -1
    assert cluster(n=(1024, 1024, 129)) == -2 and b"2^27" in lib.rsn_last_error()
    assert cluster(nbytes=16) == -4 and b"needed" in lib.rsn_last_error()
    assert lib.rsn_decimate_resolve(6, 2, 4, 4, 4, None, p, p, big, p, None) == -1
    assert lib.rsn_decimate_resolve(6, 2, 4, 0, 4, p, p, p, big, p, None) == -1
    assert lib.rsn_decimate_count(6, 2, None, 4, 4, 4, p, big, p, None) == -1
    assert lib.rsn_decimate_count(-6, 2, p, 4, 4, 4, p, big, p, None) == -1
    # the size call: 0 with a message outside the limits, and enough for the arrays the header names inside them
    assert lib.rsn_decimate_workspace_bytes(6, 2, 0, 4, 4) == 0 and b"cells" in lib.rsn_last_error()
    assert lib.rsn_decimate_workspace_bytes(-1, 2, 4, 4, 4) == 0 and lib.rsn_decimate_workspace_bytes(6, 2, 1024, 1024, 129) == 0
    assert lib.rsn_decimate_workspace_bytes(0, 0, 1, 1, 1) > 0
    assert lib.rsn_decimate_workspace_bytes(1000, 2000, 8, 8, 8) >= 4 * 512 + 4 * 1000 + 28 * 512 + 9 * 2000
    # without vertices or triangles the later calls launch nothing and need nothing
    assert lib.rsn_decimate_resolve(0, 5, 4, 4, 4, None, None, None, 0, None, None) == 0
    assert lib.rsn_decimate_count(5, 0, None, 4, 4, 4, None, 0, None, None) == 0
    assert lib.rsn_decimate_emit(0, None, 0, None, good_o, good_c, 4, 4, 4, None, 0, 0, 0, None, None, None) == 0


def test_package_argument_errors(tmp_path):
    # export_mesh refuses before it reads the checkpoint (which does not exist)
    with pytest.raises(ValueError, match="exclude each other"):
        mesh.export_mesh(str(tmp_path / "none.ckpt"), str(tmp_path / "m.ply"), decimate_cells=8, target_faces=100)
    for kw in ({"decimate_cells": 0}, {"target_faces": 0}, {"target_faces": -5}):
        with pytest.raises(ValueError, match="at least 1"):
            mesh.export_mesh(str(tmp_path / "none.ckpt"), str(tmp_path / "m.ply"), **kw)


def test_cli_flags(capsys):
    base = ["export-mesh", "--ckpt", "no-such-run", "--out", "m.ply"]
    a = trainer.build_parser().parse_args(base)
    assert (a.decimate_cells, a.target_faces) == (None, None)  # no default: omitting both is the export as it was
    a = trainer.build_parser().parse_args(base + ["--target-faces", "50000"])
    assert (a.decimate_cells, a.target_faces) == (None, 50000)
    cloud = ["export-pointcloud", "--ckpt", "no-such-run", "--out", "c.ply", "--poses", "p.json"]
    for argv, word in ((base + ["--decimate-cells", "8", "--target-faces", "100"], "exclude each other"),
                       (base + ["--decimate-cells", "0"], "--decimate-cells 0"),
                       (base + ["--target-faces", "0"], "--target-faces 0"),
                       (base + ["--target-faces", "-7"], "--target-faces -7"),
                       (base + ["--method", "tsdf", "--poses", "p.json", "--decimate-cells", "-1"], "--decimate-cells -1"),
                       (base + ["--target-faces", "10", "--resolution", "2"], "--resolution 2"),
                       (cloud + ["--target-faces", "100"], "unrecognized arguments: --target-faces"),  # no mesh route
                       (cloud + ["--decimate-cells", "8"], "unrecognized arguments: --decimate-cells")):
        with pytest.raises(SystemExit) as e:
            trainer.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    sub = [act for act in trainer.build_parser()._actions if hasattr(act, "choices") and act.choices and "export-mesh" in act.choices]
    text = " ".join(sub[0].choices["export-mesh"].format_help().split())
    assert "--decimate-cells" in text and "--target-faces" in text
