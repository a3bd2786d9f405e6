"""The distortion loss (mip-NeRF 360 eq. 15) without a GPU: the float64 reference against first principles, the O(S) prefix form of
the kernels against the O(S^2) double sum, the reference gradient against finite differences, and the host side of the feature --
ABI, argument errors (no launch), the trainer's flags and run state, the loss dictionary's refusal to drop the term."""
import ctypes as C
import os
import re

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, parallel, train_graph, train_ops, trainer
from reflect_sampling_nerf_amd._build import build_library
from tests import distortion_reference as dr
from tests.helpers import default_dtype

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX_S = (1, 2, 5, 63, 64, 65, 130, 192)


@pytest.fixture(scope="module")
def lib():
    build_library()
    return pkg.load_library()


# ------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("S", [1, 2, 5])
def test_reference_is_the_double_integral_of_the_step_density(S):
    """L_ray = int int p(u) p(v) |u - v| du dv for the piecewise-constant density p = w_i / d_i on bin i (mip-NeRF 360, eq. 14).

    Grid: the midpoint rule with N = 2048 equal cells per bin, in float64.  Between two different bins |u - v| is linear in both
    variables and the midpoint rule is exact.  Inside one bin of width d the rule gives sum_ab |a - b| (d/N)^3 = (d^3 / 3)(1 - 1/N^2)
    instead of d^3 / 3: a relative error of 1/N^2 = 2.4e-7 on the intra-bin term alone, hence below that on L_ray, under the asserted
    1e-6."""
    N = 2048
    g = torch.Generator().manual_seed(90 + S)
    with default_dtype(torch.float64):
        sb = torch.cumsum(0.05 + torch.rand(3, S + 1, generator=g, dtype=torch.float64), -1)
        sb = ((sb - sb[:, :1]) / (sb[:, -1:] - sb[:, :1])).float()  # fp32 input bits, strictly ascending on [0, 1]
        w = (torch.rand(3, S, generator=g, dtype=torch.float64) / S).float()
        ref = dr.loss_ray_reference(sb, w)
        lo, d = sb.double()[:, :-1], sb.double()[:, 1:] - sb.double()[:, :-1]
        frac = (torch.arange(N, dtype=torch.float64) + 0.5) / N
        u = (lo[:, :, None] + d[:, :, None] * frac).reshape(3, S * N)                    # cell midpoints
        mass = (w.double() / N)[:, :, None].expand(3, S, N).reshape(3, S * N)            # p du of every cell
        integral = torch.zeros(3)
        for a in range(0, S * N, 1024):  # row chunks of the [S N, S N] integrand
            integral += (mass[:, a:a + 1024, None] * mass[:, None, :] * (u[:, a:a + 1024, None] - u[:, None, :]).abs()).sum((-1, -2))
    rel = float(((integral - ref).abs() / ref).max())
    print(f"S={S}: midpoint rule vs reference {rel:.3e} relative")
    assert rel <= 1e-6


@pytest.mark.parametrize("S", PREFIX_S)
def test_prefix_form_equals_the_double_sum(S):
    """The O(S) form on prefix sums (what the kernels evaluate, here in float64) against the O(S^2) form, loss and dL/dw, on the seeded
    inputs with every planted ray: 1e-12 of the scale (the sums of non-negative terms themselves)."""
    inp = dr.distortion_inputs(37, S, dr.distortion_seed(S))
    w = dr.weights64(inp).float()  # fp32 bits, as the kernels read them
    ref = dr.loss_ray_reference(inp["sb"], w)
    got = dr.loss_ray_prefix(inp["sb"], w)
    assert bool(((got - ref).abs() <= 1e-12 * ref).all()), float(((got - ref).abs() / ref.clamp(min=1e-300)).max())
    gref = dr.g_w_reference(inp["sb"], w.double())
    ggot = dr.g_w_prefix(inp["sb"], w)
    assert bool(((ggot - gref).abs() <= 1e-12 * gref).all())
    # the planted rays are what their description says
    inter, intra = dr.loss_ray_terms(inp["sb"], w)
    assert float(ref[0]) == 0.0 and float(gref[0].abs().max()) == 0.0
    assert float(inter[1]) == 0.0 and float(intra[1]) > 0.0 and float(w[1, 0]) == 1.0 and float(w[1, 1:].abs().sum()) == 0.0
    if S > 1:
        span = float(inp["sb"][3, -1] + inp["sb"][3, -2] - inp["sb"][3, 1] - inp["sb"][3, 0]) / 2  # last midpoint - first midpoint
        assert abs(float(inter[3]) - 0.5 * span) <= 1e-6 and float(inter[3]) == float(inter.max())  # 2 (1/2)(1/2) |m_last - m_0|
        assert 0.0 < float(ref[4]) < 2 * dr.NARROW and abs(float(w[4].sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("S", [1, 2, 5, 13])
def test_reference_gradient_matches_finite_differences_and_the_closed_form(S):
    """float64 autograd through w(sigma) against a central difference of the same float64 loss (h = 1e-6: the truncation is h^2 / 6
    times a third derivative of at most delta^3 <= 4^3 per unit of loss, ~1e-11; the rounding 1e-16 |loss| / h = 1e-10; both far below
    the asserted 1e-6 of the largest entry), and against the closed form coded with plain loops."""
    inp = dr.distortion_inputs(7, S, dr.distortion_seed(S) + 1)
    grad, scale, _gw = dr.distortion_backward_reference(inp)
    closed = dr.g_sigma_closed_form(inp)
    assert bool(((closed - grad).abs() <= 1e-12 * scale + 1e-300).all())

    def total(sigma):
        return float((inp["g_loss_ray"].double() * dr.loss_ray_reference(inp["sb"], dr.weights64(inp, sigma))).sum())

    h = 1e-6
    base = inp["sigma"].double()
    fd = torch.zeros_like(base)
    for r in range(base.shape[0]):
        for k in range(S):
            e = torch.zeros_like(base)
            e[r, k] = h
            fd[r, k] = (total(base + e) - total(base - e)) / (2 * h)
    worst = float((fd - grad).abs().max()) / float(grad.abs().max())
    print(f"S={S}: finite difference vs autograd {worst:.3e} of the largest entry")
    assert worst <= 1e-6
    assert float(grad[0].abs().max()) == 0.0  # the empty ray


# ------------------------------------------------------------------------------------------------------------- ABI
def test_entry_points_are_declared_bound_and_exported(lib):
    header = open(os.path.join(REPO, "include", "rsn.h")).read()
    for name in ("rsn_distortion_forward", "rsn_distortion_backward"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"{name} is not declared in include/rsn.h"
        assert name in _abi._SIGNATURES and name in _abi.EXPORTED_SYMBOLS
        assert hasattr(lib, name)
    assert "#define RSN_ABI_VERSION 18" in header and _abi.RSN_ABI_VERSION == 18 and lib.rsn_abi_version() == 18


def test_argument_errors_are_pinned(lib):
    """Rejected before any launch (this test runs without a GPU): n_samples < 1, n_rays < 0 and, with rays to process, every NULL
    pointer other than n_dev.  n_rays == 0 is a success that launches nothing."""
    p = C.c_void_p(256)  # never dereferenced: every call below returns before a launch
    fwd, bwd = lib.rsn_distortion_forward, lib.rsn_distortion_backward
    assert fwd(4, None, 0, p, p, p, None) == -1 and b"n_samples=0" in lib.rsn_last_error()
    assert fwd(-1, None, 8, p, p, p, None) == -1 and b"n_rays=-1" in lib.rsn_last_error()
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert fwd(4, None, 8, *args, None) == -1 and b"NULL" in lib.rsn_last_error()
    assert fwd(0, None, 8, None, None, None, None) == 0
    assert bwd(4, None, 0, p, p, p, p, p, 1, None) == -1 and b"n_samples=0" in lib.rsn_last_error()
    assert bwd(-1, None, 8, p, p, p, p, p, 0, None) == -1 and b"n_rays=-1" in lib.rsn_last_error()
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert bwd(4, None, 8, *args, 1, None) == -1 and b"NULL" in lib.rsn_last_error()
    assert bwd(0, None, 8, None, None, None, None, None, 1, None) == 0
    assert bwd(4, None, 4097, p, p, p, p, p, 1, None) == -2 and b"n_samples=4097" in lib.rsn_last_error()  # one chunk total per lane


# ------------------------------------------------------------------------------------------------------------- switches and names
def test_the_term_is_off_by_default_and_the_names_stand():
    model = trainer.make_model()
    coef = model.config.loss_coefficients
    assert "distortion_loss_coarse" not in coef and "distortion_loss_fine" not in coef and len(coef) == 12
    assert train_graph.distortion_levels(model) == (False, False)
    coef["distortion_loss_fine"] = 0.0
    assert train_graph.distortion_levels(model) == (False, False)
    coef["distortion_loss_fine"] = 0.01
    assert train_graph.distortion_levels(model) == (False, True)
    coef["distortion_loss_coarse"] = 0.002
    assert train_graph.distortion_levels(model) == (True, True)
    assert len(train_graph.DIFF_KEYS) == 9 and train_graph.FUSED_KEYS == ("pn_loss_ray_coarse", "pn_loss_ray_fine", "ori_loss_ray_coarse",
                                                                         "ori_loss_ray_fine")
    assert train_graph.DIST_KEYS == ("dist_loss_ray_coarse", "dist_loss_ray_fine")
    assert train_graph.DIST_COEF_KEYS == tuple(k for k, _ in train_ops.DISTORTION_TERMS)
    assert train_graph.DIST_KEYS == tuple(k for _, k in train_ops.DISTORTION_TERMS)
    assert {"distortion_loss_coarse", "distortion_loss_fine"} <= set(parallel._MEAN_TERMS)
    assert len(train_ops.LOSS_TERMS) == 8


def test_a_set_coefficient_without_its_fused_term_raises():
    off = {"distortion_loss_fine": 0.0}
    assert train_ops.distortion_loss_dict(None, {}) == {} and train_ops.distortion_loss_dict(None, off) == {}
    assert train_ops.distortion_loss_dict({"pn_loss_ray_fine": torch.zeros(3)}, off) == {}
    with pytest.raises(_abi.RsnError, match="dist_loss_ray_fine"):
        train_ops.distortion_loss_dict(None, {"distortion_loss_fine": 0.01})
    with pytest.raises(_abi.RsnError, match="dist_loss_ray_coarse"):
        train_ops.distortion_loss_dict({"dist_loss_ray_fine": torch.ones(3)}, {"distortion_loss_fine": 0.01, "distortion_loss_coarse": 0.1})
    got = train_ops.distortion_loss_dict({"dist_loss_ray_fine": torch.tensor([1.0, 2.0, 6.0])}, {"distortion_loss_fine": 0.5})
    assert list(got) == ["distortion_loss_fine"] and float(got["distortion_loss_fine"]) == 1.5
    # through the model: outputs of a foreign path (a plain dict has no fused terms) with the coefficient set
    model = trainer.make_model()
    model.config.loss_coefficients["distortion_loss_coarse"] = 0.01
    with pytest.raises(_abi.RsnError, match="distortion_loss_coarse"):
        model.get_loss_dict({}, {"image": torch.zeros(4, 3)})


def test_parser_flags_and_defaults(capsys):
    base = ["train", "--data", "d", "--out", "o"]
    for run_defaults in (True, False):
        ap = trainer.build_parser(run_defaults)
        a = ap.parse_args(base)
        assert a.distortion_loss is None and a.distortion_loss_coarse is None
        a = ap.parse_args(base + ["--distortion-loss", "0.01"])
        assert a.distortion_loss == 0.01 and a.distortion_loss_coarse is None
        a = ap.parse_args(base + ["--distortion-loss", "0.002", "--distortion-loss-coarse", "0.001"])
        assert (a.distortion_loss, a.distortion_loss_coarse) == (0.002, 0.001)
    with pytest.raises(SystemExit):
        trainer.build_parser().parse_args(["train", "--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "0.01" in text and "0.002" in text and "neither value has been measured on this method" in text and "default: off" in text


def test_run_state_records_the_coefficients_only_when_set():
    plain = trainer.make_run_state(0, 1024, "f32", False, "cpu")
    assert set(plain) == {"version", "seed", "rays", "mma", "deterministic", "cuda_rng_state", "cpu_rng_state"}
    assert plain["version"] == trainer.RUN_STATE_VERSION == 1
    assert set(trainer.make_run_state(0, 1024, "f32", False, "cpu", distortion_loss=0.0, distortion_loss_coarse=None)) == set(plain)
    fine = trainer.make_run_state(0, 1024, "f32", False, "cpu", distortion_loss=0.01)
    assert set(fine) - set(plain) == {"distortion_loss"} and fine["distortion_loss"] == 0.01
    both = trainer.make_run_state(0, 1024, "f32", False, "cpu", distortion_loss=0.01, distortion_loss_coarse=0.002)
    assert set(both) - set(plain) == {"distortion_loss", "distortion_loss_coarse"} and both["distortion_loss_coarse"] == 0.002


def test_resolve_run_settings_given_recorded_default():
    keys = ("distortion_loss", "distortion_loss_coarse")
    none = dict.fromkeys(keys)
    cfg, notes = trainer._resolve_run_settings(none, None)
    assert cfg == none and notes == []                                    # fresh run, nothing given: off
    cfg, notes = trainer._resolve_run_settings(none, {"version": 1})
    assert cfg == none and notes == []                                    # a plain run's checkpoint records neither
    cfg, notes = trainer._resolve_run_settings(none, {"distortion_loss": 0.01})
    assert cfg == {"distortion_loss": 0.01, "distortion_loss_coarse": None} and notes == []   # recorded, not given: restored
    cfg, notes = trainer._resolve_run_settings({"distortion_loss": 0.01, "distortion_loss_coarse": 0.002}, {"distortion_loss": 0.01})
    assert cfg == {"distortion_loss": 0.01, "distortion_loss_coarse": 0.002} and notes == []  # given and equal / given and new
    cfg, notes = trainer._resolve_run_settings({"distortion_loss": 0.002, "distortion_loss_coarse": None}, {"distortion_loss": 0.01})
    assert cfg["distortion_loss"] == 0.002 and len(notes) == 1 and "not bit-exact" in notes[0]  # given wins, and is noted
