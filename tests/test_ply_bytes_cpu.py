"""mesh.write_ply and pointcloud.write_ply_points against the record of what the two separate writers wrote before they were given
one body (tests/golden/ply_bytes.json, tools/record_ply_bytes.py): a mesh, an empty mesh, a cloud and an empty cloud, each as numpy
arrays and as tensors, with colours below 0, above 1 and on the rounding rule's steps.  No byte may move, and no temporary file stay."""
import json
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN
from tools import record_ply_bytes as rec


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "ply_bytes.json")) as fh:
        return json.load(fh)


def test_the_record_covers_every_case(pinned):
    assert set(pinned) == {rec.key(s, f) for s in rec.SHAPES for f in rec.FORMS}
    for s in rec.SHAPES:
        assert pinned[rec.key(s, "numpy")] == pinned[rec.key(s, "tensor")]
    assert len({v["sha256"] for v in pinned.values()}) == len(rec.SHAPES)


def test_the_inputs_exercise_the_rounding_rule():
    diff = rec.inputs("mesh_5_2", "numpy")["diff"]
    assert diff.min() < 0.0 and diff.max() > 1.0
    steps = diff[:2].astype(np.float64) * 255.0 + 0.5
    assert np.all(np.abs(steps - np.round(steps)) < 1e-4)  # on a step up to fp32 rounding: floor decides


@pytest.mark.parametrize("form", rec.FORMS)
@pytest.mark.parametrize("shape", list(rec.SHAPES))
def test_the_writers_write_the_recorded_bytes(pinned, tmp_path, shape, form):
    assert rec.state(str(tmp_path), shape, form) == pinned[rec.key(shape, form)]
    assert os.listdir(tmp_path) == [rec.key(shape, form) + ".ply"]  # the temporary file was renamed, not left


def test_the_header_names_the_command_and_only_a_mesh_has_faces(tmp_path):
    for shape, command in (("mesh_0_0", b"export-mesh"), ("cloud_0", b"export-pointcloud")):
        rec.state(str(tmp_path), shape, "numpy")
        head = open(tmp_path / (rec.key(shape, "numpy") + ".ply"), "rb").read().split(b"\n")
        assert head[2] == b"comment reflect_sampling_nerf_amd " + command and head[-2] == b"end_header" and head[-1] == b""
        assert (b"element face 0" in head) == (shape == "mesh_0_0")
