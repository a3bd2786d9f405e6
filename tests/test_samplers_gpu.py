"""rsn_sample_spaced and rsn_sample_pdf (csrc/rsn_render.hip), called through the C ABI, against cpu_ref in float64 at the shapes where
they change path (tests/sampler_reference.py): both spacing kinds with per-ray near / far as the reflect levels use them, with and
without the random draws; one sample, a wave +- 1, several 64-entry chunks of the CDF scan at lengths that are no multiple of 64, the
limit of 1024 input bins and its refusal at 1025; flat CDF runs (histogram padding 0), all-zero weights and weights summing below
1e-5; draws of exact 0 and of 1 - 2^-24; device-side counts (rows behind them keep the poison); the grid-stride loops of both.

The rule is field_maths_reference.compare, factor 4 over the float32 oracle's own worst error plus its floor: spacing bins of the PDF
sampler scaled by 1 + slope of the inverse CDF at the sample, those of the spaced sampler absolute, Euclidean bins relative per
spacing kind and decade of far; output bins non-decreasing along every ray.  The PDF sampler's Euclidean bins are judged twice: against
cpu_ref.pdf_bins scaled by |e| + (1 + slope) |de/db| (they inherit the spacing bins' slope-amplified error through the map's
derivative; sampler_reference.judge_pdf says why an error relative to |e| alone cannot be held per case), and the map alone,
relative, on the spacing bins the kernel itself wrote.  Samples within 64 x 2^-24 of a knot adjoining a flat
CDF run are left out, at most 0.5 % of a case.  No bound is a number taken from the kernels; tests/test_samplers_cpu.py shows the
rule passing a float32 emulation and rejecting its planted faults.  Every check prints its verdict (tools/step_edges_report.py
collects them into profiles/step_edges.json).

Every output buffer is 64 rows longer than needed and filled with tests.helpers._POISON before the launch."""
import contextlib

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, ops
from reflect_sampling_nerf_amd._abi import ptr
from tests import sampler_reference as SR
from tests.helpers import _POISON, _check_count, _count, _is_poison, _poisoned

pytestmark = pytest.mark.gpu
TAIL = 64
SPACING = {"uniform": _abi.RSN_SPACING_UNIFORM, "reciprocal": _abi.RSN_SPACING_RECIPROCAL}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


_dead = []


@contextlib.contextmanager
def _launching():
    """GPU work of this file: once a launch has raised, no later test starts another one on the device."""
    if _dead:
        pytest.fail(f"an earlier launch of this file failed ({_dead[0]}): not launching again")
    try:
        yield
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        _dead.append(repr(e))
        raise


def _outputs(R, nb, dev):
    return _poisoned({"sb": torch.empty(R + TAIL, nb, device=dev), "eb": torch.empty(R + TAIL, nb, device=dev)})


def _finish(label, vs, failures):
    text = "\n".join([SR.report(v) for v in vs] + failures)
    print(text)
    assert all(v.ok for v in vs) and not failures, "\n" + text


def run_spaced(dev, c):
    """One rsn_sample_spaced launch -> (case, outputs on the device, rows that must be written)."""
    kind, R, S, jitter, live = c
    case = SR.spaced_case(kind, R, S, jitter)
    lib = _abi.load_library()
    out = _outputs(R, S + 1, dev)
    nears, fars = case["nears"].to(dev), case["fars"].to(dev)
    t_rand = None if case["t_rand"] is None else case["t_rand"].to(dev)
    with _launching():
        rc = lib.rsn_sample_spaced(R, ptr(None if live is None else _count(live, dev)), S, SPACING[kind], case["tan"], ptr(nears), ptr(fars),
                                   ptr(t_rand), ptr(out["sb"]), ptr(out["eb"]), ops._stream())
        _abi.check(rc)
    return case, out, R if live is None else live


@pytest.mark.parametrize("c", SR.SPACED_CASES, ids=SR.spaced_id)
def test_spaced_sampler_against_fp64(dev, c):
    case, out, live = run_spaced(dev, c)
    _check_count(SR.spaced_id(c), out, live)
    _finish(SR.spaced_id(c), *SR.judge_spaced(SR.spaced_id(c), case, out["sb"].cpu(), out["eb"].cpu(), live))


def run_pdf(dev, c):
    """One rsn_sample_pdf launch -> (case, outputs on the device, rows that must be written)."""
    kind, R, s_in, s_out, pad, zero, u_rand, live = c
    case = SR.pdf_case(kind, R, s_in, s_out, pad, zero, u_rand)
    lib = _abi.load_library()
    out = _outputs(R, s_out + 1, dev)
    args = [case[k].to(dev) for k in ("nears", "fars", "w", "sb_in")]
    u = None if case["u_rand"] is None else case["u_rand"].to(dev)
    with _launching():
        rc = lib.rsn_sample_pdf(R, ptr(None if live is None else _count(live, dev)), s_in, s_out, SPACING[kind], case["tan"], pad,
                                *[ptr(t) for t in args], ptr(u), ptr(out["sb"]), ptr(out["eb"]), ops._stream())
        _abi.check(rc)
    return case, out, R if live is None else live


@pytest.mark.parametrize("c", SR.PDF_CASES, ids=SR.pdf_id)
def test_pdf_sampler_against_fp64(dev, c):
    case, out, live = run_pdf(dev, c)
    _check_count(SR.pdf_id(c), out, live)
    vs, failures, share = SR.judge_pdf(SR.pdf_id(c), case, out["sb"].cpu(), out["eb"].cpu(), live)
    print(f"EXCLUDED {SR.pdf_id(c)}: {share:.4%} (cap {SR.CAP:.2%})")
    _finish(SR.pdf_id(c), vs, failures)


def test_pdf_sampler_refuses_1025_input_bins(dev):
    """s_in = 1025 is one more than the LDS arrays hold: RSN_ERR_UNSUPPORTED, rsn_last_error names the length, nothing is written."""
    lib = _abi.load_library()
    R, s_in, s_out = 5, 1025, 8
    out = _outputs(R, s_out + 1, dev)
    z = lambda *s: torch.rand(*s, device=dev)  # noqa: E731
    nears, fars, w, sb_in = z(R), z(R) + 2.0, z(R, s_in), torch.sort(z(R, s_in + 1), dim=-1).values.contiguous()
    with _launching():
        rc = lib.rsn_sample_pdf(R, None, s_in, s_out, SPACING["uniform"], 1.0, 0.01, ptr(nears), ptr(fars), ptr(w), ptr(sb_in), None,
                                ptr(out["sb"]), ptr(out["eb"]), ops._stream())
    assert rc == -2, rc  # RSN_ERR_UNSUPPORTED (include/rsn.h)
    assert b"s_in=1025" in lib.rsn_last_error(), lib.rsn_last_error()
    for k, t in out.items():
        assert bool(_is_poison(t).all()), f"{k} was written by a refused call"
    assert _POISON[torch.float32][1] == 0x7FC0DEAD
