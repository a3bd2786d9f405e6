#!/usr/bin/env python
"""Records tests/golden/packed_sha256.json: the SHA-256 of the packed weight buffer for every case of
tests/test_gpu_parity.py::test_packed_bytes_are_pinned, hashed by the test's own function, with whatever library RSN_LIBRARY
names (the build of the commit whose bytes are to be pinned).  Needs the GPU.
Usage: RSN_LIBRARY=<librsn_hip.so of that commit> python tools/record_packed_sha256.py [out.json]"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.helpers import GOLDEN  # noqa: E402
from tests.test_gpu_parity import PACKED_PIN_MODES, PACKED_PIN_SHAPES, packed_pin_key, packed_sha256  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(GOLDEN, "packed_sha256.json")
dev = torch.device("cuda:0")
pinned = {packed_pin_key(*shape, mode): packed_sha256(dev, *shape, mode) for shape in PACKED_PIN_SHAPES for mode in PACKED_PIN_MODES}
with open(out, "w") as fh:
    json.dump(pinned, fh, indent=1, sort_keys=True)
    fh.write("\n")
print("%d hashes -> %s (library: %s)" % (len(pinned), out, os.environ.get("RSN_LIBRARY", "the tree's own")))
