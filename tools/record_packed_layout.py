"""Records what the library states about its packed buffer and its saved layout, for every mode and a set of shapes, into
tests/golden/packed_layout.json: rsn_packed_weights_bytes and rsn_train_saved_layout.  No GPU is needed (neither call launches).
tests/test_packed_layout_cpu.py compares the library in the tree with the record; re-record only with a change that is meant to
move a size or a slot (RSN_LIBRARY selects another build of the same ABI).
  python tools/record_packed_layout.py [--out tests/golden/packed_layout.json]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import _abi  # noqa: E402

MODES = {"f32": _abi.RSN_MMA_F32, "bf16x6": _abi.RSN_MMA_BF16X6, "bf16x3": _abi.RSN_MMA_BF16X3, "bf16": _abi.RSN_MMA_BF16,
         "f32_folded": _abi.RSN_MMA_F32_FOLDED}
# (trunk layers, width, parameter width or 0, skip layer or -1): every width the kernels serve, the padded parameter widths, the
# depths with and without a skip, the one-layer net (no hT_seed / hT_last)
SHAPES = [(8, 256, 0, 4), (8, 256, 200, 4), (8, 128, 0, 4), (8, 128, 100, 4), (8, 64, 0, 4), (8, 64, 48, 4), (4, 128, 0, 2),
          (3, 256, 0, 1), (3, 64, 0, -1), (2, 64, 0, -1), (2, 256, 0, -1), (1, 64, 0, -1), (10, 256, 0, 4)]


def key(mode, shape):
    return f"{mode}_L{shape[0]}_w{shape[1]}_p{shape[2]}_skip{shape[3]}"


def state(lib, mode, shape):
    layers, width, param_width, skip = shape
    d = _abi.FieldDesc()
    d.num_layers, d.width, d.skip_layer, d.mid_width, d.density_bias, d.mma_mode, d.param_width = layers, width, skip, 128, 0.5, MODES[mode], \
        param_width
    enc_cols, sh_cols, narrow = C.c_int32(), C.c_int32(), C.c_int32()
    enc_map, sh_map = (C.c_int32 * 128)(), (C.c_int32 * 64)()
    rc = lib.rsn_train_saved_layout(C.byref(d), C.byref(enc_cols), C.byref(sh_cols), C.byref(narrow), enc_map, sh_map)
    return {"packed_bytes": int(lib.rsn_packed_weights_bytes(C.byref(d))), "saved_layout_rc": int(rc), "enc_cols": enc_cols.value,
            "sh_cols": sh_cols.value, "narrow_bf16": narrow.value, "enc_map": list(enc_map), "sh_map": list(sh_map)}


def record(lib):
    return {key(m, s): state(lib, m, s) for m in MODES for s in SHAPES}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "packed_layout.json"))
    a = ap.parse_args()
    with open(a.out, "w") as fh:
        json.dump(record(pkg.load_library()), fh, indent=0, sort_keys=True)
    print(f"wrote {a.out}")
