"""The samplers' rule (tests/sampler_reference.py) against itself, without a GPU: a float32 emulation of the two kernels -- its own
code, float32 throughout, the kernels' linspace and operation order -- stands in for them.  The clean emulation has to pass every
case, also with its CDF summed in float32 in another order (64-entry blocks scanned by doubling, a float32 carry); each planted
fault has to be rejected; and the share of samples the rule leaves out stays under its cap on every case, on the reference alone.

One planted fault changes nothing that a value can show, and its test pins exactly that: no_min, the CDF not clamped at 1.  The
pdf sums to 1 up to rounding, so the unclamped CDF ends within an ulp or two of 1 and moves no kept sample by more than
4 x 2^-24 (1 + slope) on any case of this suite (measured: 3.3), inside float32's own error.  Where it does move a sample by whole
bins -- u == 1.0 on a trailing flat run -- float32 and float64 already differ, and the sample is among those left out.

The flat bounds of test_gpu_parity.py::test_pdf_sampler (1e-5 on spacing bins, 2e-5 on Euclidean bins), on the same faults
(test_the_flat_bounds_on_the_same_faults): on that test's kind of case -- histogram padding 0.01, hence no flat run and no sum below
1e-5 -- searchsorted's side ("left") and the padding share ("pad_share") leave every output bit unchanged, so any bound accepts
them there (what they need is the cases), and the unclamped CDF ("no_min") is accepted as it is everywhere.  On the cases of this suite the flat bounds cannot be used
at all: they refuse the clean emulation (1.3e-5 on spacing bins where the inverse CDF is steep, 2.7e-3 on Euclidean bins with
far = 200), while at a typical sample of a padded histogram they are 80 times wider than float32 needs."""
import pytest
import torch

from tests import sampler_reference as SR

f32, f64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------- the emulation
def _linspace0(end, steps):
    """torch.linspace(0, end, steps) in float32 as the kernels evaluate it: from the start in the first half, from the end in the second."""
    if steps <= 1:
        return torch.zeros(1, dtype=f32)
    end = torch.tensor(end, dtype=f32)
    k = torch.arange(steps)
    step = end / torch.tensor(float(steps - 1), dtype=f32)
    return torch.where(k < steps // 2, step * k.float(), end - step * (steps - 1 - k).float())


def _fn(kind, tan, x):
    return x / (torch.tensor(1.0, dtype=f32) / torch.tensor(tan, dtype=f32) + x) if kind == "reciprocal" else x


def _euclid(kind, tan, b, nears, fars, swap=False):
    s_near, s_far = _fn(kind, tan, nears)[:, None], _fn(kind, tan, fars)[:, None]
    if swap:
        s_near, s_far = s_far, s_near
    x = b * s_far + (1.0 - b) * s_near
    return x / torch.tensor(tan, dtype=f32) / (1.0 - x) if kind == "reciprocal" else x


def emulate_spaced(case, mut=None):
    """mut: "unclamped_centres" (the jitter interval of the first and the last bin reaches half a step outside [0, 1]),
    "swap" (s_near and s_far exchanged)."""
    S = case["S"]
    b = _linspace0(1.0, S + 1)
    if case["t_rand"] is not None:
        k = torch.arange(S + 1)
        bl, bu = b[(k - 1).clamp(min=0)], b[(k + 1).clamp(max=S)]
        lower, upper = (b + bl) / 2.0, (bu + b) / 2.0
        if mut == "unclamped_centres":
            half = (b[1] - b[0]) / 2.0
            lower, upper = torch.where(k == 0, b - half, lower), torch.where(k == S, b + half, upper)
        b = lower + (upper - lower) * case["t_rand"]
    else:
        b = b.expand(case["R"], S + 1)
    return b.contiguous(), _euclid(case["kind"], case["tan"], b, case["nears"], case["fars"], swap=mut == "swap")


def _scan_blocked32(pdf):
    """Inclusive prefix sums in float32: 64-entry blocks scanned by doubling (the order of a wave scan), a float32 carry between them."""
    R, n = pdf.shape
    out, carry = torch.empty_like(pdf), torch.zeros(R, dtype=f32)
    for base in range(0, n, 64):
        v = torch.zeros(R, 64, dtype=f32)
        v[:, : min(64, n - base)] = pdf[:, base: base + 64]
        off = 1
        while off < 64:
            v = torch.cat([v[:, :off], v[:, off:] + v[:, :-off]], 1)
            off *= 2
        v = v + carry[:, None]
        out[:, base: base + 64] = v[:, : min(64, n - base)]
        carry = v[:, 63]
    return out


def emulate_pdf(case, mut=None, scan="f64"):
    """mut: "left" (searchsorted's side), "no_min" (the CDF not clamped at 1), "pad_share" (the padding share divided by s_in + 1),
    "no_half" (no half-bin offset of u without u_rand), "u_div_sout" (u_rand / s_out).  scan: how the CDF is summed."""
    w, sb = case["w"], case["sb_in"]
    s_in, s_out = case["s_in"], case["s_out"]
    nb = s_out + 1
    wp = w + torch.tensor(case["pad"], dtype=f32)
    wsum = wp.sum(-1, keepdim=True)
    short = (torch.tensor(1e-5, dtype=f32) - wsum).clamp(min=0.0)
    share = short / torch.tensor(float(s_in + 1 if mut == "pad_share" else s_in), dtype=f32)
    pdf = (wp + share) / (wsum + short)
    csum = torch.cumsum(pdf.double(), -1).float() if scan == "f64" else _scan_blocked32(pdf)
    if mut != "no_min":
        csum = csum.clamp(max=1.0)
    cdf = torch.cat([torch.zeros(w.shape[0], 1, dtype=f32), csum], -1).contiguous()
    u = _linspace0(1.0 - 1.0 / nb, nb).expand(w.shape[0], nb)
    if case["u_rand"] is not None:
        u = u + case["u_rand"] / torch.tensor(float(s_out if mut == "u_div_sout" else nb), dtype=f32)
    elif mut != "no_half":
        u = u + torch.tensor(1.0 / (2.0 * nb), dtype=f32)
    u = u.contiguous()
    idx = torch.searchsorted(cdf, u, right=mut != "left")
    below, above = (idx - 1).clamp(0, s_in), idx.clamp(0, s_in)
    c0, c1, b0, b1 = cdf.gather(-1, below), cdf.gather(-1, above), sb.gather(-1, below), sb.gather(-1, above)
    t = torch.nan_to_num((u - c0) / (c1 - c0), nan=0.0).clamp(0.0, 1.0)
    b = b0 + t * (b1 - b0)
    assert b.dtype == f32
    return b.contiguous(), _euclid(case["kind"], case["tan"], b, case["nears"], case["fars"])


def _ok(vs, failures):
    return all(v.ok for v in vs) and not failures


def _say(vs, failures):
    return "\n" + "\n".join([SR.report(v) for v in vs] + failures)


# ---------------------------------------------------------------------------------------------- the reference alone
@pytest.mark.parametrize("c", SR.PDF_CASES, ids=SR.pdf_id)
def test_pdf_reference_restatement_and_exclusion_cap(c):
    """pdf_details (the fp64 restatement that yields slope and the flat-run flag) reproduces cpu_ref.pdf_bins in fp64; the samples
    it flags stay under the cap; with the histogram padding on there is no flat run and nothing is flagged."""
    case = SR.pdf_case(*c[:7])
    d = case["details"]
    assert float((d["bins"] - case["ref"][0]).abs().max()) <= 1e-14
    share = SR.excluded_share(case)
    print(f"EXCLUDED {SR.pdf_id(c)}: {share:.4%} (cap {SR.CAP:.2%})")
    assert share <= SR.CAP
    if case["pad"] > 0:
        assert share == 0.0
    assert bool(torch.isfinite(d["slope"]).all()) and float(d["slope"].min()) >= 0.0


def test_the_cases_reach_what_they_are_for():
    """Lengths either side of the 64-entry chunks and the LDS limit, both paddings on the all-zero and the below-1e-5 rays, the
    stride loops, the planted draws."""
    s_ins = {c[2] for c in SR.PDF_CASES}
    assert {1, 63, 65, 130, 1024} <= s_ins and max(s_ins) == 1024
    assert {c[4] for c in SR.PDF_CASES} == {0.0, 0.01}
    assert any(c[1] > 4096 * 4 and c[0] == "reciprocal" for c in SR.PDF_CASES)
    assert any(c[1] * (c[2] + 1) > 2048 * 256 for c in SR.SPACED_CASES)
    case = SR.pdf_case("uniform", SR.R_SMALL, 65, 64, 0.0, 0.5, True)
    assert float(case["w"][0].sum()) == 0.0 and 0.0 < float(case["w"][1].sum()) < 1e-5
    assert float(case["w"][2, :16].abs().max()) == 0.0 and float(case["u_rand"][2].max()) == 0.0
    assert float(case["u_rand"][3].min()) == SR.U_LAST < 1.0
    rec = SR.spaced_case("reciprocal", SR.R_SMALL, 63, True)
    assert float(rec["nears"].max()) == 0.0 and float(rec["fars"].min()) == 0.5 and float(rec["fars"].max()) == 200.0


# ---------------------------------------------------------------------------------------------- the clean emulation
@pytest.mark.parametrize("c", SR.SPACED_CASES, ids=SR.spaced_id)
def test_clean_spaced_emulation_passes(c):
    case = SR.spaced_case(*c[:4])
    vs, failures = SR.judge_spaced(SR.spaced_id(c), case, *emulate_spaced(case))
    print(_say(vs, failures))
    assert _ok(vs, failures), _say(vs, failures)


@pytest.mark.parametrize("scan", ["f64", "blocked32"])
@pytest.mark.parametrize("c", SR.PDF_CASES, ids=SR.pdf_id)
def test_clean_pdf_emulation_passes(c, scan):
    case = SR.pdf_case(*c[:7])
    vs, failures, _ = SR.judge_pdf(f"{SR.pdf_id(c)} {scan}", case, *emulate_pdf(case, scan=scan))
    print(_say(vs, failures))
    assert _ok(vs, failures), _say(vs, failures)


# ---------------------------------------------------------------------------------------------- planted faults
PDF_FAULTS = {  # fault: the case it is planted on
    "left": ("uniform", SR.R_SMALL, 65, 64, 0.0, 0.5, True),         # ray 2: a leading flat run and u == 0
    "no_min": ("uniform", SR.R_SMALL, 130, 129, 0.0, 0.9, True),
    "pad_share": ("reciprocal", SR.R_SMALL, 65, 64, 0.0, 0.5, False),  # ray 1: weights summing below 1e-5
    "no_half": ("uniform", SR.R_SMALL, 63, 64, 0.01, 0.0, False),
    "u_div_sout": ("reciprocal", SR.R_SMALL, 63, 64, 0.01, 0.0, True),
}
SPACED_FAULTS = {"unclamped_centres": ("reciprocal", SR.R_SMALL, 63, True), "swap": ("uniform", SR.R_SMALL, 63, False)}


@pytest.mark.parametrize("mut", [m for m in PDF_FAULTS if m != "no_min"])
def test_planted_pdf_fault_is_rejected(mut):
    case = SR.pdf_case(*PDF_FAULTS[mut])
    vs, failures, _ = SR.judge_pdf(mut, case, *emulate_pdf(case, mut))
    print(_say(vs, failures))
    assert not vs[0].ok, f"{mut}: the spacing bins were accepted" + _say(vs, failures)
    assert _ok(*SR.judge_pdf("clean", case, *emulate_pdf(case))[:2]), "the same case without the fault"


@pytest.mark.parametrize("mut", list(SPACED_FAULTS))
def test_planted_spaced_fault_is_rejected(mut):
    case = SR.spaced_case(*SPACED_FAULTS[mut])
    vs, failures = SR.judge_spaced(mut, case, *emulate_spaced(case, mut))
    print(_say(vs, failures))
    assert not _ok(vs, failures), f"{mut} was accepted" + _say(vs, failures)
    assert not (vs[0].ok if mut == "unclamped_centres" else vs[1].ok)
    assert _ok(*SR.judge_spaced("clean", case, *emulate_spaced(case)))


@pytest.mark.parametrize("scan", ["f64", "blocked32"])
def test_an_unclamped_cdf_moves_no_kept_sample_beyond_rounding(scan):
    """no_min on every case: the kept samples move by at most 4 x 2^-24 (1 + slope) against the clean emulation -- below what float32
    itself does to them -- so no comparison of values rejects it, and the rule accepts it as it accepts the clean emulation."""
    worst = 0.0
    for c in SR.PDF_CASES:
        case = SR.pdf_case(*c[:7])
        d = case["details"]
        a, b = emulate_pdf(case, scan=scan)[0], emulate_pdf(case, "no_min", scan=scan)[0]
        moved = ((a.double() - b.double()).abs() / (1.0 + d["slope"]))[~d["near"]]
        worst = max(worst, float(moved.max()) / SR.EPS)
        vs, failures, _ = SR.judge_pdf(f"no_min {SR.pdf_id(c)}", case, b, emulate_pdf(case, "no_min", scan=scan)[1])
        assert _ok(vs, failures), _say(vs, failures)
    print(f"no_min ({scan}): kept samples move by at most {worst:.2f} x 2^-24 (1 + slope)")
    assert worst <= 4.0


def test_the_flat_bounds_on_the_same_faults():
    """The module docstring's statements about 1e-5 / 2e-5, measured."""
    padded = SR.pdf_case("uniform", SR.R_SMALL, 63, 64, 0.01, 0.0, True)  # test_pdf_sampler's kind of case
    clean = emulate_pdf(padded)
    for mut in ("left", "pad_share"):
        out = emulate_pdf(padded, mut)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(clean, out)), mut
    flat = lambda case, out: (float((out[0].double() - case["ref"][0]).abs()[~case["details"]["near"]].max()),  # noqa: E731
                              float((out[1].double() - case["ref"][1]).abs()[~case["details"]["near"]].max()))
    e_sb, e_eb = flat(padded, clean)
    typical = float((clean[0].double() - padded["ref"][0]).abs().median())
    assert e_sb <= 1e-5 and e_eb <= 2e-5 and typical <= 1e-5 / 80  # far wider than the clean chain needs at a typical sample ...
    steep = SR.pdf_case(*PDF_FAULTS["pad_share"])
    far = SR.pdf_case(*PDF_FAULTS["u_div_sout"])
    print(f"flat errors of the clean emulation: padded uniform {e_sb:.2e} / {e_eb:.2e}, steep {flat(steep, emulate_pdf(steep))}, "
          f"far = 200 {flat(far, emulate_pdf(far))}")
    assert flat(steep, emulate_pdf(steep))[0] > 1e-5 and flat(far, emulate_pdf(far))[1] > 2e-5  # ... and too narrow for these
