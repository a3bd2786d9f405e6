"""The single-step rule of tests/optimizer_reference.py against itself, without a GPU: a float32 emulation of rsn_radam_step -- its
own code: the step-dependent factors formed in double on the host and rounded to float32, the element update in float32 in the
kernel's operation order -- stands in for the kernel.  The clean emulation passes at every listed step, learning rate and eps, from
moments of a previous step and from fresh ones; each planted fault is rejected.

One of the planted faults changes nothing that a value can show, and its test pins exactly that instead of pretending otherwise:
  switch_ge -- the switch taken at rho_t >= 5 instead of rho_t > 5.  With beta2 = 0.999, rho_5 = 4.996 and rho_6 = 5.994: no step has
               rho_t == 5, so the fault is a no-op, bit for bit.  Its observable neighbour, the switch one step early
               (rho_t > 4: step 5 rectified), is planted beside it and is rejected.
The rectification factor off by 1e-3 relative is rejected by the rule, while twelve steps at 2e-6 absolute
(test_gpu_parity.py::test_fused_radam_matches_torch_optim) accept it: shown on that test's own inputs at the end of this file."""
import math

import pytest
import torch

from tests import optimizer_reference as O

f32, f64 = torch.float32, torch.float64
N = 4099


def factors(t, beta1, beta2, mut=None):
    """bias_c1, bias_c2_sqrt, rect (None: not rectified) in double, as the host side of the launch forms them."""
    tb = t - 1 if mut == "bias_prev" else t
    bias1, bias2 = 1.0 - beta1 ** tb, 1.0 - beta2 ** tb
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    rho_t = rho_inf - 2.0 * t * beta2 ** t / (1.0 - beta2 ** t)
    on = {"switch_ge": rho_t >= 5.0, "switch_early": rho_t > 4.0}.get(mut, rho_t > 5.0)
    rect = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) if on else None
    if rect is not None and mut == "no_rect":
        rect = 1.0
    if rect is not None and mut == "rect_1e-3":
        rect *= 1.0 + 1e-3
    return bias1, math.sqrt(bias2), rect


def emulate(p, g, m, v, t, lr, eps, mut=None):
    """One step in float32 -> (p, m, v).  mut: beta2_first (beta2 in the first moment), no_rect (no rectification above the switch),
    eps_in_sqrt (sqrt(v + eps)), bias_prev (bias corrections of step t - 1), switch_ge, switch_early, rect_1e-3."""
    c = lambda x: torch.tensor(x, dtype=f32)  # noqa: E731
    b1, b2 = c(O.BETAS[0]), c(O.BETAS[1])
    bias1, bias2_sqrt, rect = factors(t, O.BETAS[0], O.BETAS[1], mut)
    bm = b2 if mut == "beta2_first" else b1
    mi = bm * m + (1.0 - bm) * g
    vi = b2 * v + (1.0 - b2) * g * g
    mhat = mi / c(bias1)
    if rect is None:
        return p + mhat * c(lr) * -1.0, mi, vi
    root = torch.sqrt(vi + c(eps)) if mut == "eps_in_sqrt" else torch.sqrt(vi) + c(eps)
    return p + mhat * c(lr) * (c(bias2_sqrt) / root) * c(rect) * -1.0, mi, vi


def _run(st, t, lr, eps, mut=None):
    out = emulate(st["p"], st["g"], st["m"], st["v"], t, lr, eps, mut)
    assert all(x.dtype == f32 for x in out)
    return O.judge(f"{mut or 'clean'} t{t} lr{lr:.0e} eps{eps:.0e}", st, t, lr, eps, *out)


def test_the_steps_hold_both_branches_and_the_switch():
    below, above = O.switch_steps()
    assert (max(below), min(above)) == (5, 6) and 7 in above and 1 in below
    assert all(O.rho(t) != 5.0 for t in range(1, 100))
    assert 65536 in O.SIZES and 65537 in O.SIZES and max(O.SIZES) == 90880


@pytest.mark.parametrize("fresh", [False, True], ids=["previous_moments", "fresh_moments"])
@pytest.mark.parametrize("eps", O.EPSS)
@pytest.mark.parametrize("lr", O.LRS)
@pytest.mark.parametrize("t", O.STEPS)
def test_clean_step_passes(t, lr, eps, fresh):
    vs = _run(O.make_state(N, 11 + fresh, fresh), t, lr, eps)
    print(f"SHARE {O.worst_share(vs):.3f}\n" + O.report(vs))
    assert all(v.ok for v in vs), "\n" + O.report(vs)


FAULTS = [("beta2_first", 7, "radam m"), ("no_rect", 1000, "radam p"), ("eps_in_sqrt", 7, "radam p"), ("bias_prev", 7, "radam p"),
          ("switch_early", 5, "radam p"), ("rect_1e-3", 7, "radam p"), ("rect_1e-3", 1000, "radam p")]


@pytest.mark.parametrize("mut,t,quantity", FAULTS, ids=[f"{m}-t{t}" for m, t, _ in FAULTS])
def test_planted_fault_is_rejected(mut, t, quantity):
    """Each fault is rejected at the quantity it touches, and the moments it does not touch still pass."""
    vs = _run(O.make_state(N, 11), t, O.LRS[0], O.EPSS[0], mut)
    print(O.report(vs))
    by = {v.rows[0]["quantity"]: v for v in vs}
    assert not by[quantity].ok, f"{mut} at step {t} was accepted:\n" + O.report(vs)
    assert by["radam v"].ok and (by["radam m"].ok or quantity == "radam m")


def test_the_switch_at_rho_equal_to_five_is_no_fault_at_beta2_0_999():
    """rho_t >= 5 in place of rho_t > 5: no listed step, nor any other, has rho_t == 5 (rho_5 = 4.996), so the planted line changes
    no bit of any output and no comparison of values can reject it.  What a misplaced switch does show is planted as switch_early."""
    st = O.make_state(N, 11)
    for t in O.STEPS:
        a, b = emulate(st["p"], st["g"], st["m"], st["v"], t, O.LRS[0], O.EPSS[0]), emulate(st["p"], st["g"], st["m"], st["v"], t, O.LRS[0], O.EPSS[0], "switch_ge")
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), t
    assert 4.99 < O.rho(5) < 5.0 < O.rho(6) < 6.0


def test_twelve_steps_at_2e_6_accept_a_rectification_factor_off_by_1e_3():
    """test_fused_radam_matches_torch_optim's own inputs (parameters of order 1, gradients randn * (0.1 + step), lr 1e-3, eps 1e-15,
    twelve steps, 2e-6 absolute at the end): the emulation with the rectification factor 1e-3 too large stays within that bound of
    the clean one, while the single-step rule rejects it (test_planted_fault_is_rejected)."""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(256 * 99, generator=g)
    grads = [torch.randn(256 * 99, generator=g) * (0.1 + s) for s in range(12)]
    end = {}
    for mut in (None, "rect_1e-3"):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for s in range(12):
            p, m, v = emulate(p, grads[s], m, v, s + 1, O.LRS[0], O.EPSS[0], mut)
        end[mut] = p
    off = float((end[None].double() - end["rect_1e-3"].double()).abs().max())
    print(f"rect x (1 + 1e-3) over twelve steps: parameters move by {off:.3e} (the flat bound is 2e-6)")
    assert 0.0 < off <= 2e-6 / 2
