"""Records what mesh.write_ply and pointcloud.write_ply_points write for fixed inputs into tests/golden/ply_bytes.json: the SHA-256
and the length of every file.  No GPU is needed (the writers are host code).  tests/test_ply_bytes_cpu.py compares the writers in
the tree with the record, which was made before the two writers were given one body; re-record only with a change that is meant
to move a byte of the files.
  python tools/record_ply_bytes.py [--out tests/golden/ply_bytes.json]"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reflect_sampling_nerf_amd import mesh, pointcloud  # noqa: E402

SHAPES = {"mesh_5_2": (5, 2), "mesh_0_0": (0, 0), "cloud_7": (7, None), "cloud_0": (0, None)}  # (vertices, triangles or None: a cloud)
FORMS = ("numpy", "tensor")


def key(shape, form):
    return f"{shape}_{form}"


def inputs(shape, form):
    """The arrays of one case, the same for both forms.  The colours run from below 0 to above 1, and the first two rows sit on
    the rounding rule's steps, (k + 0.5) / 255: floor(c * 255 + 0.5) decides them."""
    V, T = SHAPES[shape]
    rng = np.random.default_rng(0)
    diff = rng.uniform(-0.3, 1.3, (V, 3)).astype(np.float32)
    steps = ((np.array([[0, 1, 127], [128, 253, 254]], dtype=np.float32) + np.float32(0.5)) / np.float32(255.0))[:V]
    diff[:len(steps)] = steps
    if V:
        diff[-1] = (-0.0, 1.0, 0.0)
    d = {"positions": rng.normal(size=(V, 3)).astype(np.float32), "pred_normals": rng.normal(size=(V, 3)).astype(np.float32),
         "diff": diff, "roughness": rng.uniform(size=V).astype(np.float32), "tint": rng.uniform(size=(V, 3)).astype(np.float32)}
    if T is not None:
        d["triangles"] = rng.integers(0, max(V, 1), (T, 3)).astype(np.int32)
    return {k: torch.from_numpy(v.copy()) for k, v in d.items()} if form == "tensor" else d


def state(folder, shape, form):
    """Write the case into `folder` -> {"sha256", "bytes"} of the file."""
    path = os.path.join(folder, key(shape, form) + ".ply")
    got = (mesh.write_ply if SHAPES[shape][1] is not None else pointcloud.write_ply_points)(path, inputs(shape, form))
    assert got == path
    with open(path, "rb") as fh:
        blob = fh.read()
    return {"sha256": hashlib.sha256(blob).hexdigest(), "bytes": len(blob)}


def record(folder):
    return {key(s, f): state(folder, s, f) for s in SHAPES for f in FORMS}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ply_bytes.json"))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as folder:
        rec = record(folder)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
    print(f"wrote {a.out}")
