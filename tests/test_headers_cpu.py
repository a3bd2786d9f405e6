"""The headers under csrc/ stand on their own, and a source includes only what it uses.

rsn_device_math.h (scalar maths, typedefs), rsn_gemm_loops.h (the per-wave K loops) and rsn_epilogues.h (the accumulator
epilogues) were one header once; rsn_render.hip and rsn_wgrad.hip took all of it for a handful of typedefs and sin_big.  No GPU:
hipcc only parses here."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "reflect_sampling_nerf_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))

# names of the K loops and the epilogues: none of them may be reachable from a source that runs no per-wave GEMM
LOOP_AND_EPILOGUE_NAMES = ["MmaTraits", "WBuf", "RowBuf", "sv_put", "split8", "gemm_run", "gemm_bf16", "gemm_mode", "init_acc",
                           "ReluBits", "store_act", "store_masked_bits"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("header", HEADERS)
def test_header_parses_on_its_own(header):
    cmd = [HIPCC, "-fsyntax-only", "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(REPO, "include"), "-I", CSRC,
           os.path.join(CSRC, header)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, "%s does not parse by itself:\n%s%s" % (header, res.stdout, res.stderr)


def _reachable(source):
    """The csrc/ headers `source` includes, directly or through another header."""
    seen, todo = [], [source]
    while todo:
        with open(os.path.join(CSRC, todo.pop())) as fh:
            for inc in re.findall(r'^#include "(rsn_\w+\.h)"', fh.read(), re.M):
                if inc not in seen:
                    seen.append(inc)
                    todo.append(inc)
    return seen


def test_the_split_is_the_one_the_sources_include():
    assert {"rsn_device_math.h", "rsn_gemm_loops.h", "rsn_epilogues.h"} <= set(HEADERS) and "rsn_mfma.h" not in HEADERS
    assert set(_reachable("rsn_field_kernel.h")) >= {"rsn_device_math.h", "rsn_gemm_loops.h", "rsn_epilogues.h", "rsn_field_common.h"}


@pytest.mark.parametrize("source", ["rsn_render.hip", "rsn_wgrad.hip"])
def test_no_loops_or_epilogues_behind_a_source_without_gemm_loops(source):
    headers = _reachable(source)
    assert "rsn_device_math.h" in headers
    for h in headers:
        with open(os.path.join(CSRC, h)) as fh:
            text = fh.read()
        found = [n for n in LOOP_AND_EPILOGUE_NAMES if re.search(r"\b%s\b" % n, re.sub(r"//.*", "", text))]
        assert not found, "%s reaches %s, which holds %s" % (source, h, found)
    with open(os.path.join(CSRC, source)) as fh:
        body = re.sub(r"//.*", "", fh.read())
    assert not [n for n in LOOP_AND_EPILOGUE_NAMES if re.search(r"\b%s\b" % n, body)], "the list names something %s uses" % source
