"""GPU checks of the decimation: rsn_decimate_* through decimate.py against the numpy restatement of include/rsn.h
(tests/decimate_reference.py), by bits and order -- closed and open inputs, an anisotropic grid of cells, a mesh of 10^5 vertices
whose loops take several trips and whose scans several tiles, constructed groups, special values, empty inputs --, the face-budget
search against its restatement, and the route from a checkpoint to a file through the command line."""
import json
import math

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import decimate, mesh, render, trainer
from tests import decimate_reference as ref
from tests import helpers
from tests.mesh_reference import parse_ply
from tests.test_decimate_cpu import CELL, DIMS, ORIGIN, SPECIAL, constructed

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def on_device(pos, tri):
    return {"positions": torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32)).to(DEV).reshape(-1, 3),
            "triangles": torch.from_numpy(np.ascontiguousarray(tri).astype(np.int32)).to(DEV).reshape(-1, 3)}


def assert_equal_by_bits(got, want):
    """got: decimate.decimate's dict; want: decimate_reference.decimate's."""
    st = got["stats"]
    assert (st["vertices"], st["triangles"], st["degenerate"], st["cancelled_pairs"]) == tuple(want["counts"])
    assert st["occupied_cells"] == want["occupied"]
    assert set(got) == {"positions", "triangles", "stats"}
    assert got["positions"].dtype == torch.float32 and got["triangles"].dtype == torch.int32
    pos, tri = got["positions"].cpu().numpy(), got["triangles"].cpu().numpy()
    assert pos.shape == want["positions"].shape and tri.shape == want["triangles"].shape
    assert np.array_equal(tri, want["triangles"])
    assert np.array_equal(pos.view(np.int32), want["positions"].view(np.int32))


def frame_bounds(dims, origin, cell):
    """Bounds whose pointcloud.cell_frame is exactly (dims, origin, cell), for frames of small binary numbers."""
    o, c = np.asarray(origin, np.float64), np.asarray(cell, np.float64)
    return tuple(o) + tuple(o + c * np.asarray(dims, np.float64))


@pytest.mark.parametrize("name, cells", [("sphere_33", 3), ("sphere_33", 5), ("sphere_33", 8), ("sphere_33", 16), ("torus_33", 5),
                                         ("torus_33", 12), ("gyroid", (4, 7, 3))])
def test_equal_to_the_reference_by_bits(name, cells):
    pos, tri = ref.fixture_mesh(name)
    bounds = ref.GYROID_BOX if name == "gyroid" else ref.BOX
    dims, origin, cell = ref.cell_frame(bounds, cells)
    want = ref.decimate(pos, tri, origin, cell, dims)
    got = decimate.decimate(on_device(pos, tri), bounds, cells)
    torch.cuda.synchronize()
    print(name, cells, got["stats"])
    assert want["counts"][1] > 0
    assert got["stats"]["cells"] == list(dims) and got["stats"]["triangles_in"] == len(tri)
    assert_equal_by_bits(got, want)


@pytest.fixture(scope="module")
def large_sphere():
    """The suite's sphere on a 129^3 grid, from the device extractor (an input, not a result under test): about 10^5 vertices and
    2 x 10^5 triangles, so every grid-stride loop over triangles takes a second trip (past 262,144) and every scan several tiles."""
    shape, origin, spacing = ref.box_grid(129)
    m = mesh.extract_surface(torch.from_numpy(ref.sphere_volume(129)).to(DEV), 0.0, origin, spacing)
    torch.cuda.synchronize()
    assert m["positions"].shape[0] > 90000 and m["triangles"].shape[0] > 180000
    return m, m["positions"].cpu().numpy(), m["triangles"].cpu().numpy().astype(np.int64)


def test_multi_block_shape(large_sphere):
    m, pos, tri = large_sphere
    dims, origin, cell = ref.cell_frame(ref.BOX, 32)
    want = ref.decimate(pos, tri, origin, cell, dims)
    a = decimate.decimate(m, ref.BOX, 32)
    b = decimate.decimate(m, ref.BOX, 32)
    torch.cuda.synchronize()
    print(a["stats"])
    assert want["counts"][1] > 4000
    assert_equal_by_bits(a, want)
    for k in ("positions", "triangles"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert a["stats"] == b["stats"]
    assert ref.edge_imbalance(a["triangles"].cpu().numpy()) == 0


@pytest.mark.parametrize("copies", ["++-", "-++", "++", "+-", "+", "--+--"])
def test_constructed_groups(copies):
    pos, tri = constructed(copies)
    assert_equal_by_bits(decimate.decimate(on_device(pos, tri), frame_bounds(DIMS, ORIGIN, CELL), DIMS), ref.decimate(pos, tri, ORIGIN, CELL, DIMS))


def test_indices_out_of_range_and_shared_cells_are_degenerate():
    pos, _ = constructed("+")
    tri = np.asarray([[0, 1, 3], [0, 1, 2], [-1, 1, 2], [0, 2 ** 31 - 1, 2], [0, 0, 1], [-2 ** 31, 1, 2]], np.int64)
    want = ref.decimate(pos, tri, ORIGIN, CELL, DIMS)
    assert want["counts"] == (3, 1, 5, 0)
    assert_equal_by_bits(decimate.decimate(on_device(pos, tri), frame_bounds(DIMS, ORIGIN, CELL), DIMS), want)


def test_special_value_positions():
    """Every pair of the special coordinates of the CPU file as (x, y) of a vertex, on four cells per axis from 0: the cells and
    the means of NaN, the infinities, the faces and the outside.  Triangles join consecutive vertices."""
    x, y = np.meshgrid(SPECIAL, SPECIAL, indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), np.resize(SPECIAL[::-1], x.size)], axis=1).astype(np.float32)
    tri = np.stack([np.arange(len(pos) - 2), np.arange(1, len(pos) - 1), np.arange(2, len(pos))], axis=1)
    dims, origin, cell = (4, 4, 4), np.zeros(3, np.float32), np.ones(3, np.float32)
    want = ref.decimate(pos, tri, origin, cell, dims)
    assert want["counts"][1] > 0 and np.all(np.isfinite(want["positions"]))
    assert_equal_by_bits(decimate.decimate(on_device(pos, tri), frame_bounds(dims, origin, cell), dims), want)


def test_empty_inputs_one_cell_and_one_cell_per_axis():
    pos, tri = ref.fixture_mesh("sphere_24")
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    for p, t in ((none_v, none_t), (pos, none_t), (none_v, tri[:5])):  # V = 0 and T = 0 launch nothing
        got = decimate.decimate(on_device(p, t), ref.BOX, 4)
        st = got["stats"]
        assert (st["vertices"], st["triangles"], st["degenerate"], st["cancelled_pairs"], st["occupied_cells"]) == (0, 0, 0, 0, 0)
        assert got["positions"].shape == (0, 3) and got["triangles"].shape == (0, 3)
    for cells in (1, (1, 1, 1)):  # one cell per axis: everything is degenerate
        got = decimate.decimate(on_device(pos, tri), ref.BOX, cells)
        dims, origin, cell = ref.cell_frame(ref.BOX, cells)
        assert_equal_by_bits(got, ref.decimate(pos, tri, origin, cell, dims))
        assert got["stats"]["degenerate"] == len(tri) and got["stats"]["triangles"] == 0 and got["stats"]["vertices"] == 0
    # all vertices in one cell of a grid of many
    small = (pos * np.float32(0.01) + np.float32(0.1)).astype(np.float32)
    got = decimate.decimate(on_device(small, tri), ref.BOX, 8)
    assert (got["stats"]["occupied_cells"], got["stats"]["vertices"], got["stats"]["triangles"]) == (1, 0, 0)
    assert got["positions"].shape == (0, 3) and got["triangles"].shape == (0, 3)


def test_more_occupied_cells_than_the_key_holds_is_refused():
    """130^3 = 2,197,000 vertices at the centres of as many cells: more than the 2^21 ranks three of which share a sort key.  The
    calls run through without grouping anything, the package refuses, and a probe reports the grid as one that cannot be run.
    The same vertices in 128^3 cells occupy exactly 2^21 of them, the most that runs."""
    n = 130
    i = torch.arange(n, device=DEV, dtype=torch.float32) + 0.5
    z, y, x = torch.meshgrid(i, i, i, indexing="ij")
    pos = torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], dim=1).contiguous()
    tri = torch.arange(3000, device=DEV, dtype=torch.int32).reshape(1000, 3)  # three neighbours along x: three cells each
    m, bounds = {"positions": pos, "triangles": tri}, (0.0, 0.0, 0.0, float(n), float(n), float(n))
    with pytest.raises(pkg.RsnError, match="2\\^21"):
        decimate.decimate(m, bounds, n)
    assert decimate.survivors(m, bounds, n) is None
    got = decimate.decimate(m, bounds, 128)  # 128^3 cells: at most 2^21 occupied
    assert got["stats"]["occupied_cells"] == 128 ** 3 and got["stats"]["triangles"] + got["stats"]["degenerate"] == 1000


_reference_survivors = {}


@pytest.mark.parametrize("target", [200, 2000, 50000])
def test_search(large_sphere, target):
    m, pos, tri = large_sphere
    max_cells = 128

    def count(n):  # the reference's probes, shared among the three budgets
        if n not in _reference_survivors:
            _reference_survivors[n] = ref.survivors(pos, tri, ref.BOX, n)
        return _reference_survivors[n]

    n, probes, over = ref.search_cells(count, target, max_cells)
    want, want_st = ref.decimate(pos, tri, *ref.cell_frame(ref.BOX, n)[1:], (n, n, n)), {"n": n, "probes": probes, "over_budget": over}
    got, st = decimate.decimate_to(m, ref.BOX, target, max_cells)
    torch.cuda.synchronize()
    print(target, st)
    assert st["n"] == want_st["n"] and st["probes"] == [list(p) for p in want_st["probes"]] and st["over_budget"] == want_st["over_budget"]
    assert not st["over_budget"] and st["triangles"] <= target and st["target_faces"] == target and st["max_cells"] == max_cells
    assert set(got) == {"positions", "triangles"}
    got["stats"] = st
    assert_equal_by_bits(got, want)


# ---------------------------------------------------------------------------------------------- checkpoint -> file
RES, BOUNDS, SIDE, FOV_DEG = 24, (-1.2, -1.2, -1.2, 1.2, 1.2, 1.2), 16, 40.0


@pytest.fixture(scope="module")
def small_run(tmp_path_factory):
    """The small random model of tests/test_mesh_gpu.py as a run directory, and the median of its density as the level."""
    cfg = pkg.ReflectSamplingNeRFModelConfig(base_mlp_num_layers=4, base_mlp_layer_width=64)
    model = trainer.make_model(cfg, seed=3).to(DEV).eval()
    run = str(tmp_path_factory.mktemp("decimate") / "run")
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    trainer.save_checkpoint(trainer.checkpoint_path(run, 7), model, opt, 7)
    return run, float(mesh.density_grid(model.field, BOUNDS, RES, mma="f32").median())


def test_export_mesh_with_a_face_budget_through_the_cli(small_run, tmp_path, capsys):
    run, iso = small_run
    common = ["--ckpt", run, "--resolution", str(RES), "--bounds", *[str(b) for b in BOUNDS]]
    out = str(tmp_path / "a.ply")
    argv = ["export-mesh", "--out", out, "--iso", repr(iso), "--target-faces", "300", *common]
    assert trainer.main(argv) == 0
    line = capsys.readouterr().out.strip().split("\n")[-1]
    res = mesh.export_mesh(run, str(tmp_path / "b.ply"), resolution=RES, bounds=BOUNDS, iso=iso, target_faces=300)
    d = res["decimate"]
    print(res)
    assert 0 < res["triangles"] <= 300 and res["triangles"] == d["triangles"] and res["vertices"] == d["vertices"]
    assert res["triangles_extracted"] == d["triangles_in"] > 300 and res["vertices_extracted"] == d["vertices_in"]
    assert d["max_cells"] == RES - 1 and 2 <= d["n"] <= RES - 1 and d["probes"] and not d["over_budget"]
    assert set(res["seconds"]) == {"grid", "count", "emit", "decimate", "attributes", "write"}
    assert f"{res['vertices']} vertices, {res['triangles']} triangles" in line and "clustered from" in line
    assert open(out, "rb").read() == open(res["out"], "rb").read()  # two runs write identical files
    vert, faces, _ = parse_ply(out)
    assert len(vert["x"]) == res["vertices"] and faces.shape == (res["triangles"], 3)
    assert faces.min() == 0 and faces.max() == res["vertices"] - 1 and len(np.unique(faces)) == res["vertices"]  # valid, all used
    pos = np.stack([vert["x"], vert["y"], vert["z"]], 1)
    assert np.all(np.isfinite(pos)) and np.all(np.abs(pos) <= np.float32(1.2) * (1 + 2 ** -22))
    # --decimate-cells, and the other two routes with the budget: they complete, and the budget holds
    assert trainer.main(["export-mesh", "--out", str(tmp_path / "c.ply"), "--iso", repr(iso), "--decimate-cells", "6", *common]) == 0
    assert parse_ply(str(tmp_path / "c.ply"))[1].shape[0] < res["triangles_extracted"]
    assert trainer.main(["export-mesh", "--out", str(tmp_path / "t.obj"), "--iso", repr(iso), "--target-faces", "300", "--texture", *common]) == 0
    obj = open(tmp_path / "t.obj").read().split("\n")
    assert sum(ln.startswith("f ") for ln in obj) == res["triangles"]
    c2w = render.orbit_path(4, (0.0, 0.0, 0.0), 4.0, 20.0)
    frames = [{"file_path": f"./{i}", "transform_matrix": np.vstack([m, [[0, 0, 0, 1]]]).tolist()} for i, m in enumerate(np.asarray(c2w, np.float64))]
    poses = tmp_path / "poses.json"
    poses.write_text(json.dumps({"camera_angle_x": math.radians(FOV_DEG), "w": SIDE, "h": SIDE, "frames": frames}))
    # the tsdf route on the fog model of tests/test_tsdf_gpu.py, whose depth maps have a surface inside the box (the random model's have none)
    _, fog = helpers.fog_checkpoint(tmp_path / "fog", DEV)
    tsdf = ["export-mesh", "--method", "tsdf", "--ckpt", fog, "--resolution", str(RES), "--poses", str(poses)]
    assert trainer.main([*tsdf, "--out", str(tmp_path / "full.ply")]) == 0
    assert trainer.main([*tsdf, "--out", str(tmp_path / "s.ply"), "--target-faces", "300"]) == 0
    full, few = parse_ply(str(tmp_path / "full.ply"))[1], parse_ply(str(tmp_path / "s.ply"))[1]
    print("tsdf route:", len(full), "->", len(few), "triangles")
    assert len(full) > 300 and 0 < len(few) <= 300 and len(np.unique(few)) == few.max() + 1
