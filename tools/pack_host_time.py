#!/usr/bin/env python
"""Host time of a weight re-pack (8 x 256, skip 4): Field.packed_weights() after an in-place parameter update -- same
pointers, so the job table is not rebuilt -- and the bare rsn_pack_weights_table call beneath it.  The device is idle when
the clock starts; the clock stops when the call returns (the launches are enqueued, not finished).  Median over --calls.
Usage: [RSN_LIBRARY=<.so>] python tools/pack_host_time.py [--calls 1000] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import reflect_sampling_nerf_amd as pkg  # noqa: E402
from reflect_sampling_nerf_amd import ops  # noqa: E402
from reflect_sampling_nerf_amd._abi import check, load_library, ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=1000)
ap.add_argument("--json", default=None)
args = ap.parse_args()
lib = load_library()
dev = torch.device("cuda:0")
res = {"library": os.environ.get("RSN_LIBRARY", "tree"), "calls": args.calls}
for mode in ("f32", "bf16x6"):
    torch.manual_seed(0)
    fld = pkg.ReflectSamplingNeRFNerfField().to(dev)
    fld.set_mma_mode(mode)
    fld.packed_weights()
    w = fld.mlp_base.layers[0].weight
    desc, ps = fld.field_desc(), fld._param_struct()
    nbytes, tbytes = fld._packed.numel() * 4, fld._pack_table.numel()
    field_us, abi_us = [], []
    for i in range(args.calls + 50):
        with torch.no_grad():
            w.add_(0.0)  # bumps the version: packed_weights() packs again
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fld.packed_weights()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        check(lib.rsn_pack_weights_table(C.byref(desc), C.byref(ps), ptr(fld._packed), nbytes, ptr(fld._pack_table), tbytes, 0,
                                         ops._stream()))
        t3 = time.perf_counter()
        if i >= 50:
            field_us.append((t1 - t0) * 1e6)
            abi_us.append((t3 - t2) * 1e6)
    torch.cuda.synchronize()
    res[mode] = {"field_packed_weights_us_median": round(statistics.median(field_us), 2),
                 "rsn_pack_weights_table_us_median": round(statistics.median(abi_us), 2)}
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(res, fh)
