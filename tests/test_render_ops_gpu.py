"""The ray-level kernels around the field (rsn_render.hip, rsn_train_ops.hip), each called directly through the C ABI and compared with
float64 references that share nothing with them (tests/render_reference.py: cpu_ref + float64 autograd for compositing, the formulas
of include/rsn.h for the rest), at the shapes where they change path: one lane / a full wave +- 1 / several 64-sample chunks, the
grid-stride ray loops, the 1024-ray blocks of the reflect compaction, the single-workgroup loss reduction, device-side counts.
Every output buffer starts as tests.helpers._POISON, so "not written" and "written behind the count" both show."""
import ctypes as C

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, ops, train_graph
from reflect_sampling_nerf_amd._abi import CompositeBwdIO, CompositeIO, ReflectIO, check, ptr
from reflect_sampling_nerf_amd.train_ops import _ptr_array
from tests import render_reference as rr
from tests.helpers import _check_count, _count, _is_poison, _poisoned, default_dtype, max_abs

pytestmark = pytest.mark.gpu

EPS = rr.EPS
# Outputs that are sums of rounded products: |error against fp64| / scale, the scale being the fp64 sum of the absolute values of the terms
# the output adds (render_reference.composite_reference; a sum of same-signed terms is its own scale).  Worst ratio measured on MI355X
# over all cases of this file, in units of 2^-24, and the bound at 4x that (the convention of test_multitile_gpu.py's constants).
# CEILING is derived, not measured: each term carries a handful of fp32 roundings and one expf, the long scans run in fp64.
# What fp32 does to exp(-X) by rounding X itself (up to X 2^-24 relative: 32 x 2^-24 for an optical depth of 32) is allowed on top of the
# bound, from the fp64 depths (render_reference.composite_reference, `depth`); without that allowance g_sigma, g_color, weights and
# ori_loss_ray measure 19 - 25 x 2^-24, all of it on rays whose transmittance is below 1e-7.
# g_sigma with the scale taken literally as delta_k (|g_w[k]| T_{k+1} + sum_{i>k} |g_w[i]| w_i) measures 5899 x 2^-24: g_w[k] is a sum of
# up to five rounded products of either sign (g_c (colour_c - bg_c), g_rough roughness, g_acc), and behind the last dense sample nothing
# but g_w[k] is left in the scale; the scale used here takes g_w's own terms by absolute value and equals the literal one wherever they
# share a sign (always without a background).  The literal ratio is printed next to the asserted one.
CEILING = 64 * EPS
SUM_BOUNDS = {  # name: (measured / 2^-24, bound / 2^-24)
    "g_sigma": (8.96, 35.8),
    "g_color": (7.07, 28.2),
    "g_roughness_sample": (6.51, 26.0),
    "g_bg": (1.53, 6.1),
    "weights": (6.56, 26.2),
    "rgb": (2.39, 9.5),
    "accumulation": (1.73, 6.9),
    "roughness": (0.048, 0.19),
    "pn_loss_ray": (4.36, 17.4),
    "ori_loss_ray": (6.36, 25.4),
    "losses8": (2.72, 10.8),
    "loss_fb_losses8": (2.42, 9.6),
    "ray_sum": (1.74, 6.9),
    "colsum": (1.49, 5.9),
}
assert all(4 * m >= b >= m and b * EPS <= CEILING for m, b in SUM_BOUNDS.values())
WORST = {}  # name -> worst ratio seen in this run (printed per check; the constants above come from these lines)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------- comparisons
def _check_sum(label, name, got, ref, scale, keep=None, depth=None):
    """(|got - ref| - 2^-24 depth) / scale <= SUM_BOUNDS[name] on the rows `keep` (bool [rows] or None = all).  depth: fp32's own
    rounding of the optical depth inside exp(-X) (render_reference.composite_reference), None where no exponential is involved."""
    got, ref, scale = got.detach().double().cpu(), ref.double(), scale.double()
    depth = torch.zeros_like(scale) if depth is None else depth.double()
    if keep is not None:
        got, ref, scale, depth = got[keep], ref[keep], scale[keep], depth[keep]
    assert not bool(torch.isnan(got).any()), f"{label} {name}: NaN (an element was not written, or the kernel produced one)"
    ratio = float((((got - ref).abs() - EPS * depth).clamp(min=0) / scale).max()) / EPS if got.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    bound = SUM_BOUNDS[name][1]
    print(f"RATIO {name} {ratio:.3f} [{label}] (bound {bound}, worst so far {WORST[name]:.3f})")
    assert ratio <= bound, f"{label} {name}: {ratio:.2f} x 2^-24 of the scale > {bound}"


def _check_chain(label, name, got, ref, n, keep=None, absolute=False):
    """Outputs that are a fixed short chain of fp32 operations: |got - ref| <= n 2^-24 |ref| (absolute: <= n 2^-24), n = the number of
    roundings in the formula.  fp32's denormal range adds F32_TINY."""
    got, ref = got.detach().double().cpu(), ref.double()
    if keep is not None:
        got, ref = got[keep], ref[keep]
    assert not bool(torch.isnan(got).any()), f"{label} {name}: NaN (an element was not written)"
    tol = n * EPS * (torch.ones_like(ref) if absolute else ref.abs()) + rr.F32_TINY
    worst = float(((got - ref).abs() / tol).max()) if got.numel() else 0.0
    print(f"CHAIN {name} {worst * n:.3f} of {n} roundings [{label}]")
    assert worst <= 1.0, f"{label} {name}: {worst * n:.2f} x 2^-24 relative > {n}"


def _exclusion(label, what, near, cap, R):
    n = int(near.sum())
    print(f"EXCLUDED {label}: {n} of {R} rays ({what}), cap {cap * R:.2f}")
    assert n <= cap * R, f"{label}: {n} rays excluded ({what}), cap {cap * R:.2f}"
    return ~near


# ------------------------------------------------------------------------------------------------------------- compositing
_CACHE = {}


def _composite_case(R, S, seed, dev):
    """Inputs on the host and the device, and the forward's weights (what the backward reads), once per (R, S, seed)."""
    key = (R, S, seed)
    if key not in _CACHE:
        inp = rr.composite_inputs(R, S, seed)
        d = {k: v.to(dev) for k, v in inp.items()}
        _CACHE.clear()  # one case at a time: the big one is tens of MB
        _CACHE[key] = (inp, d, {})
    return _CACHE[key]


def _forward_weights(case, R, S, background, dev):
    inp, d, memo = case
    if background not in memo:
        memo[background] = ops.composite(R, None, S, background, 0, d["sigma"], d["eb"], d["color"], bg_rgb=d["bg"],
                                         want_depth=False)["weights"]
    return memo[background]


def _composite_backward(case, R, S, background, flags, detach, dev, n_dev=None, drop=()):
    """rsn_composite_backward into poisoned buffers; `drop`: names of optional inputs / outputs passed as NULL."""
    lib = _abi.load_library()
    inp, d, _ = case
    w = _forward_weights(case, R, S, background, dev)
    out = {"g_sigma": torch.empty(R, S, device=dev), "g_color": torch.empty(R, S, 3, device=dev),
           "g_roughness_sample": torch.empty(R, S, device=dev), "g_bg": torch.empty(R, 3, device=dev)}
    if background != 2:
        del out["g_bg"]  # include/rsn.h: g_bg belongs to background == 2
    out = _poisoned({k: v for k, v in out.items() if k not in drop and not (k == "g_roughness_sample" and "roughness" in drop)})
    io = CompositeBwdIO()
    io.sigma, io.euclid_bins, io.color, io.bg_rgb = ptr(d["sigma"]), ptr(d["eb"]), ptr(d["color"]), ptr(d["bg"])
    io.weights, io.g_rgb = ptr(w), ptr(d["g_rgb"])
    io.roughness = None if "roughness" in drop else ptr(d["roughness"])
    io.g_roughness = None if "g_roughness" in drop else ptr(d["g_rough"])
    io.g_accumulation = None if "g_accumulation" in drop else ptr(d["g_acc"])
    for k in ("g_sigma", "g_color", "g_roughness_sample", "g_bg"):
        setattr(io, k, ptr(out.get(k)))
    check(lib.rsn_composite_backward(R, ptr(n_dev), S, background, flags, detach, C.byref(io), ops._stream()))
    torch.cuda.synchronize()
    return out


def _check_composite_backward(label, case, out, R, background, flags, detach, live=None, drop=()):
    inp = case[0]
    clip = bool(flags & ops.RSN_COMP_CLIP_RGB)
    ref, scale, depth = rr.composite_reference(inp, background, bool(detach), clip, use_rough="roughness" not in drop,
                                               use_g_rough="g_roughness" not in drop, use_g_acc="g_accumulation" not in drop)
    live = R if live is None else live
    keep = _exclusion(label, "clip mask", ref["clip_near"], rr.CLIP_CAP, R)
    keep[live:] = False
    _check_count(label, out, live)
    for k, got in out.items():
        if k == "g_sigma" and detach:
            assert bool((got[:live] == 0).all()), f"{label}: detached weights must give g_sigma == 0 exactly"
            continue
        _check_sum(label, k, got, ref[k], scale[k], keep, depth[k])
    if "g_sigma" in out and not detach:  # the scale as the issue writes it, with |g_w[k]| itself: equal without a background
        lit = float(((out["g_sigma"].double().cpu() - ref["g_sigma"]).abs()[keep] / scale["g_sigma_literal"][keep]).max()) / EPS
        print(f"RATIO g_sigma_literal {lit:.3f} [{label}]")
    return ref, scale, depth


@pytest.mark.parametrize("S", rr.COMPOSITE_S)
@pytest.mark.parametrize("flags", [0, ops.RSN_COMP_CLIP_RGB], ids=["noclip", "clip"])
@pytest.mark.parametrize("detach", [0, 1])
@pytest.mark.parametrize("background", [0, 1, 2])
def test_composite_backward_matches_fp64_autograd(dev, background, detach, flags, S):
    """g_sigma, g_color, g_roughness_sample, g_bg of every ray against fp64 autograd, the planted rays included (empty, saturated, a
    zero-width bin, composites exactly on the clip bounds, whose gradient must pass)."""
    R = rr.COMPOSITE_R
    case = _composite_case(R, S, rr.composite_seed(S, background), dev)
    label = f"bwd bg{background} detach{detach} flags{flags} S{S}"
    out = _composite_backward(case, R, S, background, flags, detach, dev)
    ref = _check_composite_backward(label, case, out, R, background, flags, detach)[0]
    if flags:  # the gradient passes at equality (torch.clamp's backward)
        assert bool((ref["unclipped"][3] == 1.0).all())
        assert float(out["g_color"][3, 0].min()) > 0.2, "colour == 1 composites to exactly 1.0: its gradient must pass the clip"
        if background != 1 and float(ref["weights"][4].max()) > 0:
            assert float(out["g_color"][4].abs().max()) > 0, "colour == 0 composites to exactly 0.0: its gradient must pass the clip"


OPTIONAL = ["g_roughness", "roughness", "g_accumulation", "g_sigma", "g_color", "g_roughness_sample", "g_bg"]


@pytest.mark.parametrize("drop", [(k,) for k in OPTIONAL] + [("g_roughness", "roughness", "g_accumulation")],
                         ids=OPTIONAL + ["no_optional_input"])
def test_composite_backward_optional_pointers(dev, drop):
    """Each optional input absent and each output NULL in turn: the others are unchanged against the matching fp64 loss."""
    R, S, background = rr.COMPOSITE_R, 65, 2
    case = _composite_case(R, S, rr.composite_seed(S, background), dev)
    out = _composite_backward(case, R, S, background, ops.RSN_COMP_CLIP_RGB, 0, dev, drop=drop)
    assert not (set(drop) & set(out))
    _check_composite_backward(f"bwd without {'+'.join(drop)}", case, out, R, background, ops.RSN_COMP_CLIP_RGB, 0, drop=drop)


@pytest.mark.parametrize("detach", [0, 1])
def test_composite_backward_wrapper_want_bg(dev, detach):
    """train_graph._composite_backward as the training step calls it (want_bg, per-sample roughness, g_acc)."""
    R, S, background = rr.COMPOSITE_R, 130, 2
    case = _composite_case(R, S, rr.composite_seed(S, background), dev)
    inp, d, _ = case
    w = _forward_weights(case, R, S, background, dev)
    out = train_graph._composite_backward(R, S, background, 0, detach, {"sigma": d["sigma"], "color": d["color"]}, d["eb"], w,
                                          d["g_rgb"], bg=d["bg"], g_rough=d["g_rough"], want_sigma=True, want_bg=True,
                                          rough_samples=d["roughness"], g_acc=d["g_acc"])
    torch.cuda.synchronize()
    ref, scale, depth = rr.composite_reference(inp, background, bool(detach), False)
    for k, name in (("g_color", "g_color"), ("g_rough", "g_roughness_sample"), ("g_bg", "g_bg")):
        _check_sum(f"wrapper detach{detach}", name, out[k], ref[name], scale[name], depth=depth[name])
    if detach:
        assert bool((out["g_sigma"] == 0).all())
    else:
        _check_sum("wrapper", "g_sigma", out["g_sigma"], ref["g_sigma"], scale["g_sigma"], depth=depth["g_sigma"])


@pytest.mark.parametrize("background,flags,detach", [(0, 0, 0), (2, ops.RSN_COMP_CLIP_RGB, 0), (1, 0, 1)])
def test_composite_backward_device_count(dev, background, flags, detach):
    """A device-side count of 29 in buffers for 37: rows < 29 written and right, rows >= 29 of every output untouched."""
    R, S, live = rr.COMPOSITE_R, 65, rr.COMPOSITE_LIVE
    case = _composite_case(R, S, rr.composite_seed(S, background), dev)
    out = _composite_backward(case, R, S, background, flags, detach, dev, n_dev=_count(live, dev))
    assert len(out) == (4 if background == 2 else 3)
    _check_composite_backward(f"bwd count bg{background}", case, out, R, background, flags, detach, live=live)


@pytest.mark.parametrize("background,flags", [(0, ops.RSN_COMP_CLIP_RGB), (2, 0)])
def test_composite_backward_grid_stride(dev, background, flags):
    """R = 32768 + 7: the grid is capped at 8192 blocks of 4 rays, every wave walks a second ray and the last round is ragged."""
    R, S = rr.BIG_R, rr.BIG_S
    case = _composite_case(R, S, rr.composite_seed(S, background) + 1, dev)
    out = _composite_backward(case, R, S, background, flags, 0, dev)
    ref, scale, depth = _check_composite_backward(f"bwd grid-stride bg{background}", case, out, R, background, flags, 0)
    for r in (0, 32767, 32768, R - 1):  # first ray, last of round 0, first and last of round 1
        if not bool(ref["clip_near"][r]):
            err = ((out["g_sigma"][r].double().cpu() - ref["g_sigma"][r]).abs() - EPS * depth["g_sigma"][r]) / scale["g_sigma"][r]
            assert float(err.max()) <= SUM_BOUNDS["g_sigma"][1] * EPS, f"ray {r}"


def _composite_forward_direct(d, R, S, background, flags, dev, n_dev=None):
    """rsn_composite with every output requested, into poisoned buffers."""
    lib = _abi.load_library()
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out = _poisoned({"weights": f(R, S), "rgb": f(R, 3), "accumulation": f(R), "depth": f(R), "diff_out": f(R, 3), "tint_out": f(R, 3),
                     "normals_out": f(R, 3), "roughness_out": f(R), "pn_loss_ray": f(R), "ori_loss_ray": f(R)})
    io = CompositeIO()
    io.sigma, io.euclid_bins, io.color, io.bg_rgb = ptr(d["sigma"]), ptr(d["eb"]), ptr(d["color"]), ptr(d["bg"])
    io.diff, io.tint, io.pred_normals, io.roughness = ptr(d["color"]), ptr(d["color"]), ptr(d["pred_normals"]), ptr(d["roughness"])
    io.normals, io.n_dot_d = ptr(d["normals"]), ptr(d["n_dot_d"])
    for k, v in out.items():
        setattr(io, k, ptr(v))
    check(lib.rsn_composite(R, ptr(n_dev), S, background, flags, C.byref(io), ops._stream()))
    torch.cuda.synchronize()
    return out


def _check_composite_forward(label, inp, out, background, clip, live):
    ref, scale, depth = rr.composite_reference(inp, background, False, clip)
    pn, ori, e2, nd2 = rr.ray_losses_reference(inp, ref["weights"])
    tt, xw = scale["weights"], depth["weights"]
    keep = torch.zeros(inp["sigma"].shape[0], dtype=torch.bool)
    keep[:live] = True
    for k in ("weights", "rgb", "accumulation"):
        _check_sum(label, k, out[k], ref[k], scale[k], keep, depth[k])
    if "roughness_out" in out:
        _check_sum(label, "roughness", out["roughness_out"], ref["roughness"], scale["roughness"], keep, depth["roughness"])
    _check_sum(label, "pn_loss_ray", out["pn_loss_ray"], pn, (tt * e2).sum(-1) + rr.F32_TINY, keep, (xw * e2).sum(-1))
    _check_sum(label, "ori_loss_ray", out["ori_loss_ray"], ori, (tt * nd2).sum(-1) + rr.F32_TINY, keep, (xw * nd2).sum(-1))


@pytest.mark.parametrize("background", [0, 2])
def test_composite_forward_grid_stride_and_ray_losses(dev, background):
    """rsn_composite at R = 32768 + 7 (through ops.composite, as the training graph calls it) with the fused per-ray normal losses:
    pn_loss_ray = sum_s w |n - pn|^2, ori_loss_ray = sum_s w max(0, n.d)^2, all rays."""
    R, S = rr.BIG_R, rr.BIG_S
    inp, d, _ = _composite_case(R, S, rr.composite_seed(S, background) + 1, dev)
    out = ops.composite(R, None, S, background, ops.RSN_COMP_CLIP_RGB, d["sigma"], d["eb"], d["color"], bg_rgb=d["bg"],
                        level={k: d[k] for k in ("normals", "pred_normals", "n_dot_d")}, ray_losses=True)
    torch.cuda.synchronize()
    _check_composite_forward(f"fwd grid-stride bg{background}", inp, out, background, True, R)


@pytest.mark.parametrize("background", [0, 1, 2])
def test_composite_forward_device_count(dev, background):
    """A device-side count of 29 in buffers for 37, every output of rsn_composite requested."""
    R, S, live = rr.COMPOSITE_R, 65, rr.COMPOSITE_LIVE
    inp, d, _ = _composite_case(R, S, rr.composite_seed(S, background), dev)
    out = _composite_forward_direct(d, R, S, background, 0, dev, n_dev=_count(live, dev))
    _check_count(f"fwd count bg{background}", out, live)
    _check_composite_forward(f"fwd count bg{background}", inp, out, background, False, live)


# ------------------------------------------------------------------------------------------------------------- reflect setup
REFLECT_FAR = 4.0


def _reflect_setup_direct(inp, dev):
    lib = _abi.load_library()
    R = inp["origins"].shape[0]
    d = {k: v.to(dev) for k, v in inp.items()}
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out = _poisoned({"mask": torch.empty(R, device=dev, dtype=torch.uint8), "n_masked": torch.empty(1, device=dev, dtype=torch.int32),
                     "ray_index": torch.empty(R, device=dev, dtype=torch.int32), "n_dot_d": f(R), "origins2": f(R, 3),
                     "directions2": f(R, 3), "sqradius": f(R), "pixel_area2": f(R), "nears2": f(R), "fars2": f(R),
                     "reflect_coarse": f(R, 3), "reflect_fine": f(R, 3)})
    io = ReflectIO()
    for k in ("origins", "directions", "accumulation", "depth", "pred_normals", "roughness"):
        setattr(io, k, ptr(d[k]))
    for k, v in out.items():
        setattr(io, k, ptr(v))
    ws = torch.empty(max(1, lib.rsn_reflect_workspace_bytes(R) // 4), device=dev, dtype=torch.int32)
    io.workspace = ptr(ws)
    check(lib.rsn_reflect_setup(R, REFLECT_FAR, C.byref(io), ops._stream()))
    torch.cuda.synchronize()
    return d, out


def _check_reflect_setup(label, inp, planted, out):
    """-> (mask bool [R] as the kernel wrote it, M, ray_index int64 [M]) after every check of case 3."""
    R = inp["origins"].shape[0]
    ref, near = rr.reflect_reference(inp, planted, REFLECT_FAR)
    _exclusion(label, "reflect mask", near, rr.MASK_CAP, R)
    got_mask = out["mask"].cpu()
    assert bool(((got_mask == 0) | (got_mask == 1)).all()), f"{label}: mask holds something other than 0 / 1"
    got_mask = got_mask.bool()
    ref_mask = torch.where(near, got_mask, ref["mask"])  # a ray within 1e-6 of a threshold may fall on either side
    assert bool((got_mask == ref_mask).all()), f"{label}: mask differs at rays {(got_mask != ref_mask).nonzero().flatten().tolist()[:8]}"
    M = int(out["n_masked"].item())
    assert M == int(ref_mask.sum()), f"{label}: n_masked {M}, mask has {int(ref_mask.sum())}"
    idx_ref = ref_mask.nonzero().flatten()
    assert bool((out["ray_index"][:M].cpu().long() == idx_ref).all()), f"{label}: ray_index is not mask.nonzero() (stable order)"
    compact = {k: out[k] for k in ("ray_index", "origins2", "directions2", "sqradius", "pixel_area2", "nears2", "fars2")}
    _check_count(label, compact, M)
    # n.d: 3 products and 2 additions of same-signed terms = 5 roundings
    _check_chain(label, "n_dot_d", out["n_dot_d"], ref["n_dot_d"], 5)
    dflt = ref["reflect_default"][:, None].expand(R, 3)
    for k in ("reflect_coarse", "reflect_fine"):  # white * (1 - acc): one fp32 subtraction, bit-exact on every ray
        assert bool((out[k].cpu() == dflt).all()), f"{label} {k}: not 1 - acc"
    if M:
        # origins + depth * directions (same-signed): 1 product + 1 addition = 2 roundings
        _check_chain(label, "origins2", out["origins2"][:M], ref["origins2"][idx_ref], 2)
        # unit vectors through a square root and a divide: 8 x 2^-24 absolute
        _check_chain(label, "directions2", out["directions2"][:M], ref["directions2"][idx_ref], 8, absolute=True)
        # 2 |n.d| roughness^2: n.d (5) + roughness^2 (1) + their product (1) = 7 roundings; the factor 2 is exact
        _check_chain(label, "sqradius", out["sqradius"][:M], ref["sqradius"][idx_ref], 7)
        # pi * sqradius: + fp32 pi (1) + the product (1) = 9 roundings
        _check_chain(label, "pixel_area2", out["pixel_area2"][:M], ref["pixel_area2"][idx_ref], 9)
        assert bool((out["nears2"][:M] == 0).all()) and bool((out["fars2"][:M] == REFLECT_FAR).all())
    return got_mask, M, idx_ref


@pytest.mark.parametrize("pattern", rr.REFLECT_PATTERNS)
@pytest.mark.parametrize("R", rr.REFLECT_R)
def test_reflect_setup_matches_fp64(dev, R, pattern):
    """mask, n_masked, ray_index exact (stable compaction across 1024-ray blocks), compacted rows < M against fp64, rows >= M untouched,
    the default reflect colours and n.d on every ray; threshold rays planted exactly on and one step past each threshold."""
    inp, planted = rr.reflect_inputs(R, pattern, rr.reflect_seed(R, pattern))
    _, out = _reflect_setup_direct(inp, dev)
    mask, M, _ = _check_reflect_setup(f"reflect R{R} {pattern}", inp, planted, out)
    if planted:
        a, b, c, d_ = planted
        assert not mask[a] and mask[b] and not mask[c] and mask[d_], "planted threshold rays"
        assert float(out["n_dot_d"][c]) == 0.0 and float(out["n_dot_d"][d_]) == -2.0 ** -20


def test_reflect_setup_wrapper_equals_direct_call(dev):
    R = 1025
    inp, planted = rr.reflect_inputs(R, "random", rr.reflect_seed(R, "random"))
    d, out = _reflect_setup_direct(inp, dev)
    w = ops.reflect_setup(d["origins"], d["directions"], d["accumulation"], d["depth"], d["pred_normals"], d["roughness"], REFLECT_FAR)
    torch.cuda.synchronize()
    M = int(out["n_masked"].item())
    assert int(w["n_masked"].item()) == M
    for k in ("mask", "n_dot_d", "reflect_coarse", "reflect_fine"):
        assert torch.equal(w[k], out[k]), k
    for k in ("ray_index", "origins2", "directions2", "sqradius", "pixel_area2", "nears2", "fars2"):
        assert torch.equal(w[k][:M], out[k][:M]), k


# ------------------------------------------------------------------------------------------------------------- reflect combine & backwards
@pytest.mark.parametrize("R,pattern", [(1025, "random"), (3001, "random"), (1025, "none")])
@pytest.mark.parametrize("drop", [None, "g_sqradius", "g_pixel_area"])
def test_reflect_combine_and_backwards(dev, R, pattern, drop):
    """rsn_reflect_combine, rsn_reflect_combine_backward, rsn_reflect_backward, rsn_reflect_default_backward on the ray_index / n_masked
    rsn_reflect_setup produced (M = 0 included)."""
    lib = _abi.load_library()
    inp, planted = rr.reflect_inputs(R, pattern, rr.reflect_seed(R, pattern))
    d, su = _reflect_setup_direct(inp, dev)
    label = f"combine R{R} {pattern} drop {drop}"
    mask, M, idx = _check_reflect_setup(label, inp, planted, su)
    assert (M == 0) == (pattern == "none")
    ci = rr.combine_inputs(R, 7000 + R, idx)
    g = {k: v.to(dev) for k, v in ci.items() if k != "exact"}
    ref = rr.combine_reference(ci, idx)
    keep = _exclusion(label, "combine clip", ref["near"], rr.CLIP_CAP, max(M, 1))
    # combine: scattered; rays that are not reflected keep what the buffer held
    out = _poisoned({"out": torch.empty(R, 3, device=dev)})["out"]
    ops.reflect_combine(R, su["n_masked"], su["ray_index"], g["diff"], g["tint"], g["comp"], out)
    g_comp = _poisoned({"g_comp": torch.empty(R, 3, device=dev)})["g_comp"]
    check(lib.rsn_reflect_combine_backward(R, ptr(su["n_masked"]), ptr(su["ray_index"]), ptr(g["diff"]), ptr(g["tint"]), ptr(g["comp"]),
                                           ptr(g["g_out"]), ptr(g_comp), ops._stream()))
    g_rough = _poisoned({"g": torch.empty(R, device=dev)})["g"]
    gsq = None if drop == "g_sqradius" else g["g_sqradius"]
    gpa = None if drop == "g_pixel_area" else g["g_pixel_area"]
    check(lib.rsn_reflect_backward(R, ptr(su["n_masked"]), ptr(su["ray_index"]), ptr(su["n_dot_d"]), ptr(d["roughness"]), ptr(gsq),
                                   ptr(gpa), ptr(g_rough), ops._stream()))
    g_acc = _poisoned({"g": torch.empty(R, device=dev)})["g"]
    check(lib.rsn_reflect_default_backward(R, ptr(su["mask"]), ptr(g["g_coarse"]), ptr(g["g_fine"]), ptr(g_acc), ops._stream()))
    torch.cuda.synchronize()
    untouched = _is_poison(out)
    assert bool((untouched == ~mask).all()), f"{label}: combine wrote a ray that is not reflected, or skipped one that is"
    _check_count(label, {"g_comp": g_comp}, M)
    if M:
        # diff + tint * comp, same-signed: 1 product + 1 addition = 2 roundings; then the clip
        _check_chain(label, "combine", out[idx.to(dev)], ref["out"], 2, keep)
        # g_out * tint: 1 rounding, or exactly zero outside [0, 1]
        _check_chain(label, "g_comp", g_comp[:M], ref["g_comp"], 1, keep)
        zero_ref = (ref["g_comp"] == 0)[keep]
        assert bool(((g_comp[:M].cpu() == 0)[keep] == zero_ref).all()), f"{label}: clip mask of the combine's backward"
        if M >= 2:  # exactly 1 and exactly 0 pass the gradient
            assert out[int(idx[0])].tolist() == [1.0, 0.0, 0.0] and out[int(idx[1])].tolist() == [1.0, 1.0, 1.0]
            assert float(g_comp[:2].min()) > 0, "v == 0 and v == 1 exactly: torch.clip passes the gradient"
    # reflect_backward: (g_sq + pi g_pa) * 2|n.d| * 2 roughness on reflected rays, exactly zero elsewhere
    with default_dtype(torch.float64):
        ndd32, rough = su["n_dot_d"].double().cpu(), inp["roughness"].double()
        gs = (0 if gsq is None else ci["g_sqradius"].double()[:M]) + np.pi * (0 if gpa is None else ci["g_pixel_area"].double()[:M])
        gr_ref = torch.zeros(R)
        gr_ref[idx] = gs * 2 * ndd32[idx].abs() * 2 * rough[idx]
        ga_ref = torch.where(mask, torch.zeros(()), -(ci["g_coarse"].double().sum(-1) + ci["g_fine"].double().sum(-1)))
    assert bool((g_rough.cpu()[~mask] == 0).all()), f"{label}: g_roughness of a ray that is not reflected must be exactly zero"
    # fp32 pi (1) + pi * g_pa (1) + the sum (1, same-signed) + two products (2) = 5 roundings; factors of 2 are exact
    _check_chain(label, "reflect_backward", g_rough, gr_ref, 5)
    # two 3-term sums (2 + 2), their sum (1) = 5 roundings of same-signed terms; exactly zero on reflected rays
    assert bool((g_acc.cpu()[mask] == 0).all())
    _check_chain(label, "reflect_default_backward", g_acc, ga_ref, 5)


# ------------------------------------------------------------------------------------------------------------- per-ray losses
def _loss_rays(li_dev, coef, dev, null_k=None):
    lib = _abi.load_library()
    R = li_dev["image"].shape[0]
    losses = _poisoned({"l": torch.empty(8, device=dev)})["l"]
    g = [None if k == null_k else _poisoned({"g": torch.empty(R, 3, device=dev)})["g"] for k in range(4)]
    check(lib.rsn_loss_rays_forward(R, ptr(li_dev["image"]), _ptr_array(li_dev["rgb4"]), _ptr_array(li_dev["pn_ray2"]),
                                    _ptr_array(li_dev["ori_ray2"]), (C.c_float * 8)(*coef), ptr(losses), _ptr_array(g), ops._stream()))
    torch.cuda.synchronize()
    return losses, g


@pytest.mark.parametrize("R", rr.LOSS_R)
def test_loss_rays_forward_backward_match_fp64(dev, R):
    """The eight terms and g_rgb4 of rsn_loss_rays_forward (one workgroup of 1024 threads: 3R crosses it between 341 and 342; 4099 is a
    ragged multi-pass), a NULL g_rgb4 entry, bit-identical losses8 over two calls, and rsn_loss_rays_backward's chain rule."""
    lib = _abi.load_library()
    li = rr.loss_rays_inputs(R, 8000 + R)
    ld = {k: (v.to(dev) if torch.is_tensor(v) else [t.to(dev) for t in v]) for k, v in li.items()}
    l_ref, g_ref = rr.loss_rays_reference(li, rr.LOSS_COEF)
    losses, g = _loss_rays(ld, rr.LOSS_COEF, dev)
    _check_sum(f"loss_rays R{R}", "losses8", losses, l_ref, l_ref + rr.F32_TINY)
    for k in range(4):  # coef * 2 exact, rgb - image (1), 1 / (3R) (1), two products (2) = 4 roundings
        _check_chain(f"loss_rays R{R}", f"g_rgb4[{k}]", g[k], g_ref[k], 4)
    losses2, g2 = _loss_rays(ld, rr.LOSS_COEF, dev, null_k=2)
    assert torch.equal(losses.view(torch.int32), losses2.view(torch.int32)), "losses8 must repeat bit for bit"
    for k in (0, 1, 3):
        assert torch.equal(g[k], g2[k]), "a NULL g_rgb4 entry must not change the others"
    # backward: g_rgb4[k] *= upstream8[k] (1 rounding on the fp32 bits the forward wrote); g_pn / g_ori = coef * upstream (1 rounding)
    up = torch.tensor(rr.LOSS_UPSTREAM, device=dev)
    before = [t.double().cpu() for t in g]
    g_pn = [_poisoned({"g": torch.empty(R, device=dev)})["g"] for _ in range(2)]
    g_ori = [_poisoned({"g": torch.empty(R, device=dev)})["g"], None]
    check(lib.rsn_loss_rays_backward(R, ptr(up), (C.c_float * 8)(*rr.LOSS_COEF), _ptr_array(g), _ptr_array(g_pn), _ptr_array(g_ori),
                                     ops._stream()))
    torch.cuda.synchronize()
    c32 = [float(np.float32(c)) for c in rr.LOSS_COEF]
    for k in range(4):
        _check_chain(f"loss_rays_backward R{R}", f"g_rgb4[{k}]", g[k], before[k] * rr.LOSS_UPSTREAM[k], 1)
    for lv in range(2):
        _check_chain(f"loss_rays_backward R{R}", f"g_pn_ray2[{lv}]", g_pn[lv], torch.full((R,), c32[4 + lv] * rr.LOSS_UPSTREAM[4 + lv]), 1)
    _check_chain(f"loss_rays_backward R{R}", "g_ori_ray2[0]", g_ori[0], torch.full((R,), c32[6] * rr.LOSS_UPSTREAM[6]), 1)


@pytest.mark.parametrize("R,Sc,Sf", [(5, 3, 7), (300, 130, 33), (2049, 128, 2)])
def test_loss_scale_grads_on_fused_loss_buffers(dev, R, Sc, Sf):
    """rsn_loss_forward_backward's terms and gradients against fp64 at ragged shapes, then rsn_loss_scale_grads on the buffers it wrote:
    one rounding per element.  (2049, 128, 2): 262,272 work items against the grid's cap of 1024 blocks x 256 threads, so that the
    stride loop of both kernels runs, with the three colour channels wider than the fine level.

    losses8 is a fixed-order fp64 sum of the blocks' partial sums, rounded once (rsn_loss_reduce_kernel), so it holds the recorded
    bound at 1024 blocks as at one, and a second call repeats it bit for bit."""
    lib = _abi.load_library()
    g = torch.Generator().manual_seed(R)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    image, rgb = rand(R, 3), [rand(R, 3) for _ in range(4)]
    S2 = (Sc, Sf)
    w = [rand(R, s) for s in S2]
    nrm, pn, ndd = [rand(R, s, 3) - 0.5 for s in S2], [rand(R, s, 3) - 0.5 for s in S2], [rand(R, s) - 0.5 for s in S2]
    to = lambda ts: [t.to(dev) for t in ts]  # noqa: E731
    d_rgb, d_w, d_nrm, d_pn, d_ndd = to(rgb), to(w), to(nrm), to(pn), to(ndd)
    losses = _poisoned({"l": torch.empty(8, device=dev)})["l"]
    g_rgb = [_poisoned({"g": torch.empty(R, 3, device=dev)})["g"] for _ in range(4)]
    g_pn = [_poisoned({"g": torch.empty(R, s, 3, device=dev)})["g"] for s in S2]
    g_ndd = [_poisoned({"g": torch.empty(R, s, device=dev)})["g"] for s in S2]
    check(lib.rsn_loss_forward_backward(R, Sc, Sf, ptr(image.to(dev)), _ptr_array(d_rgb), _ptr_array(d_w), _ptr_array(d_nrm),
                                        _ptr_array(d_pn), _ptr_array(d_ndd), (C.c_float * 8)(*rr.LOSS_COEF), ptr(losses),
                                        _ptr_array(g_rgb), _ptr_array(g_pn), _ptr_array(g_ndd), ops._stream()))
    losses_again = _poisoned({"l": torch.empty(8, device=dev)})["l"]
    check(lib.rsn_loss_forward_backward(R, Sc, Sf, ptr(image.to(dev)), _ptr_array(d_rgb), _ptr_array(d_w), _ptr_array(d_nrm),
                                        _ptr_array(d_pn), _ptr_array(d_ndd), (C.c_float * 8)(*rr.LOSS_COEF), ptr(losses_again),
                                        _ptr_array(g_rgb), _ptr_array(g_pn), _ptr_array(g_ndd), ops._stream()))
    torch.cuda.synchronize()
    assert torch.equal(losses.view(torch.int32), losses_again.view(torch.int32)), "losses8 must repeat bit for bit"
    label = f"loss_forward_backward R{R}"
    c = [float(np.float32(v)) for v in rr.LOSS_COEF]
    with default_dtype(torch.float64):
        img = image.double()
        l_ref = [((t.double() - img) ** 2).sum() / (3 * R) for t in rgb]
        l_ref += [(w[lv].double() * ((nrm[lv].double() - pn[lv].double()) ** 2).sum(-1)).sum() for lv in range(2)]
        l_ref += [(w[lv].double() * ndd[lv].double().clamp(min=0) ** 2).sum() for lv in range(2)]
        l_ref = torch.stack(l_ref)
    _check_sum(label, "loss_fb_losses8", losses, l_ref, l_ref + rr.F32_TINY)
    for k in range(4):  # as rsn_loss_rays_forward: 4 roundings
        _check_chain(label, f"g_rgb4[{k}]", g_rgb[k], c[k] * 2 * (rgb[k].double() - image.double()) / (3 * R), 4)
    for lv in range(2):
        # coef * w (1), n - pn (1), their product (1) = 3 roundings; the factor -2 is exact
        _check_chain(label, f"g_pn[{lv}]", g_pn[lv], c[4 + lv] * w[lv].double()[..., None] * -2 * (nrm[lv].double() - pn[lv].double()), 3)
        # coef * w (1), times 2 max(0, n.d) (1) = 2 roundings
        _check_chain(label, f"g_ndd[{lv}]", g_ndd[lv], c[6 + lv] * w[lv].double() * 2 * ndd[lv].double().clamp(min=0), 2)
    before = [[t.double().cpu() for t in grp] for grp in (g_rgb, g_pn, g_ndd)]
    up = torch.tensor(rr.LOSS_UPSTREAM, device=dev)
    check(lib.rsn_loss_scale_grads(R, Sc, Sf, ptr(up), _ptr_array(g_rgb), _ptr_array(g_pn), _ptr_array(g_ndd), ops._stream()))
    torch.cuda.synchronize()
    label = f"loss_scale_grads R{R}"
    for k in range(4):
        _check_chain(label, f"g_rgb4[{k}]", g_rgb[k], before[0][k] * rr.LOSS_UPSTREAM[k], 1)
    for lv in range(2):
        _check_chain(label, f"g_pn[{lv}]", g_pn[lv], before[1][lv] * rr.LOSS_UPSTREAM[4 + lv], 1)
        _check_chain(label, f"g_ndd[{lv}]", g_ndd[lv], before[2][lv] * rr.LOSS_UPSTREAM[6 + lv], 1)


# ------------------------------------------------------------------------------------------------------------- ray and column sums
def _ray_sum_direct(x, R, S, dev, n_dev=None):
    lib = _abi.load_library()
    out = _poisoned({"o": torch.empty(R, device=dev)})["o"]
    check(lib.rsn_ray_sum(R, ptr(n_dev), S, ptr(x), ptr(out), ops._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("S", [1, 63, 64, 65, 130])
def test_ray_sum_with_device_count(dev, S):
    R, live = 37, 29
    x = torch.randn(R, S, generator=torch.Generator().manual_seed(S))
    xd = x.to(dev)
    out = _ray_sum_direct(xd, R, S, dev, n_dev=_count(live, dev))
    _check_count(f"ray_sum S{S}", {"out": out}, live)
    keep = torch.arange(R) < live
    _check_sum(f"ray_sum S{S}", "ray_sum", out, x.double().sum(-1), x.double().abs().sum(-1) + rr.F32_TINY, keep)
    wrapped = train_graph._ray_sum(xd, R, S, n_dev=_count(live, dev))  # the training graph's wrapper: rows behind the count stay zero
    torch.cuda.synchronize()
    assert torch.equal(wrapped[:live], out[:live]) and bool((wrapped[live:] == 0).all())


def test_ray_sum_grid_stride(dev):
    R, S = rr.BIG_R, 3
    x = torch.randn(R, S, generator=torch.Generator().manual_seed(3))
    out = _ray_sum_direct(x.to(dev), R, S, dev)
    _check_sum("ray_sum grid-stride", "ray_sum", out, x.double().sum(-1), x.double().abs().sum(-1) + rr.F32_TINY)


@pytest.mark.parametrize("n_cols", [1, 3, 256, 300])
@pytest.mark.parametrize("n_rows", [0, 1, 3, 2047, 2048, 2049, 5000])
def test_colsum(dev, n_rows, n_cols):
    """out[c] (+)= sum_r x[r * ld + c] with ld = n_cols + 5 and the pad columns at 1e30 (reading them shows); accumulate 0 overwrites
    whatever the buffer held, accumulate 1 adds to a non-zero buffer.  2048 rows per block; the 4-way unroll has a tail."""
    lib = _abi.load_library()
    ld = n_cols + 5
    g = torch.Generator().manual_seed(n_rows * 1000 + n_cols)
    x = torch.full((max(n_rows, 1), ld), 1e30)
    x[:, :n_cols] = torch.randn(max(n_rows, 1), n_cols, generator=g)
    start = torch.randn(n_cols + 5, generator=g)
    xd = x.to(dev)
    live = x[:n_rows, :n_cols].double()
    for accumulate in (0, 1):
        out = start.clone().to(dev)
        check(lib.rsn_colsum(n_rows, n_cols, ld, ptr(xd), ptr(out), accumulate, ops._stream()))
        torch.cuda.synchronize()
        base = start[:n_cols].double() * accumulate
        _check_sum(f"colsum {n_rows}x{n_cols} acc{accumulate}", "colsum", out[:n_cols], base + live.sum(0),
                   base.abs() + live.abs().sum(0) + rr.F32_TINY)
        assert torch.equal(out[n_cols:].cpu(), start[n_cols:]), "colsum wrote past n_cols"


# ------------------------------------------------------------------------------------------------------------- PDF sampler
def _pdf_case(R, s_in, s_out, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(R, s_in, 1, generator=g) ** 4
    w[0] = 0.0
    w[1, : s_in // 2] = 0.0
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    sb_in, _ = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, s_in, None)
    u = torch.rand(R, s_out + 1, generator=g)
    with default_dtype(torch.float64):  # the reference in fp64 on the fp32 input bits
        sb_ref, eb_ref = cpu_ref.pdf_bins("uniform", 1.0, nears.double(), fars.double(), w.double(), sb_in.double(), s_out, u.double())
    return w, nears, fars, sb_in, u, sb_ref, eb_ref


def _pdf_direct(case, R, s_in, s_out, dev, n_dev=None):
    lib = _abi.load_library()
    w, nears, fars, sb_in, u, _, _ = case
    out = _poisoned({"sb": torch.empty(R, s_out + 1, device=dev), "eb": torch.empty(R, s_out + 1, device=dev)})
    args = [t.contiguous().to(dev) for t in (nears.reshape(R), fars.reshape(R), w[..., 0], sb_in, u)]
    check(lib.rsn_sample_pdf(R, ptr(n_dev), s_in, s_out, _abi.RSN_SPACING_UNIFORM, 1.0, 0.01,
                             *[ptr(t) for t in args], ptr(out["sb"]), ptr(out["eb"]), ops._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("R,live,s_in,s_out", [(29, 21, 64, 33), (16384 + 5, None, 7, 9)],
                         ids=["device_count", "grid_stride"])
def test_pdf_sampler_device_count_and_grid_stride(dev, R, live, s_in, s_out):
    """rsn_sample_pdf with a device-side count (21 of 29) and at R = 16384 + 5 (4096 blocks x 4 rays: the grid-stride loop), against
    cpu_ref.pdf_bins in fp64 at test_pdf_sampler's tolerances."""
    case = _pdf_case(R, s_in, s_out, 9000 + R)
    out = _pdf_direct(case, R, s_in, s_out, dev, n_dev=None if live is None else _count(live, dev))
    live = R if live is None else live
    _check_count(f"pdf R{R}", out, live)
    sb, eb = out["sb"][:live].cpu(), out["eb"][:live].cpu()
    e_sb, e_eb = max_abs(sb, case[5][:live]), max_abs(eb, case[6][:live])
    print(f"pdf R{R}: spacing bins {e_sb:.3e} (1e-5), euclidean bins {e_eb:.3e} (2e-5)")
    assert e_sb <= 1e-5  # inverse CDF amplifies 1-ulp cdf differences by 1/pdf (test_pdf_sampler)
    assert e_eb <= 2e-5
    assert bool((sb[:, 1:] >= sb[:, :-1]).all()), "resampled bins must be sorted"
