"""The size of the packed buffer and the saved layout, every mode and shape, against the record of the library as it was before
the folded backward sweep got the pieces of wT_x[L-1] (tests/golden/packed_layout.json, tools/record_packed_layout.py): those
pieces live in a region the folded buffer already had (RsnPackedLayout::hT_last = hT_bh), so no size and no slot may move.
No GPU: neither call launches anything."""
import json
import os

import pytest

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd._build import build_library
from tests.helpers import GOLDEN
from tools import record_packed_layout as rec


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLDEN, "packed_layout.json")) as fh:
        return json.load(fh)


def test_the_record_covers_every_mode_and_shape(pinned):
    assert set(pinned) == {rec.key(m, s) for m in rec.MODES for s in rec.SHAPES}
    assert all(v["packed_bytes"] > 0 and v["saved_layout_rc"] == 0 for v in pinned.values())


@pytest.mark.parametrize("mode", list(rec.MODES))
def test_packed_bytes_and_saved_layout_are_the_recorded_ones(lib, pinned, mode):
    for shape in rec.SHAPES:
        assert rec.state(lib, mode, shape) == pinned[rec.key(mode, shape)], rec.key(mode, shape)
