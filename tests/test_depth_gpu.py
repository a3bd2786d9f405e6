"""Depth supervision on the GPU: rsn_depth_loss_forward / _backward, rsn_gather_ray_depth and rsn_depth_error called through the C ABI
against the float64 references of tests/depth_reference.py at the shapes where the kernels change path (one lane, a full wave +- 1,
ragged 64-sample chunks, the grid-stride ray loop, a device-side count), then the term inside the whole training step against float64
autograd through the oracle's sigma, the loss dictionary, parallel.train_step, the trainer, and `eval --depth` end to end on the
sphere with analytic depth maps.  Every output buffer starts as tests.helpers._POISON."""
import math

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, metrics, ops, train_graph, train_ops, trainer
from reflect_sampling_nerf_amd._abi import check, ptr
from reflect_sampling_nerf_amd.data import BlenderScene, RayDataManager
from tests import capture_reference as cr
from tests import depth_reference as dz
from tests import lens_reference as lr
from tests import render_reference as rr
from tests.helpers import _POISON, _poisoned
from tests.test_gpu_parity import _loss_from_outputs, _train_setup
from tests.test_resume_gpu import _differing, _load, _Run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = rr.EPS
# |got - fp64 reference| / scale in units of 2^-24, the convention of test_distortion_gpu.py: the scale is the fp64 sum of the absolute
# values of the terms the output adds (depth_reference: L_ray's terms; g_sigma: l_k (|g_w[k]| T_{k+1} + sum_{i>k} |g_w[i]| w_i)).
# The bound is derived, not measured: both kernels are fp64 inside and round to fp32 once, which gives at most 1 x 2^-24 of the value
# and so of the scale; the factor 4 is headroom.  A ratio above it is a kernel defect.  Worst ratios measured on MI355X over all cases
# of this file (the RATIO lines these tests print; profiles/depth_loss.json): loss_ray 0.987, g_sigma 0.999.
BOUND = dz.BOUND / EPS  # 4
WORST = {}

S_CASES = rr.COMPOSITE_S            # (1, 63, 64, 65, 130, 192): one lane, a wave +- 1, ragged chunks
R_CASE, LIVE = rr.COMPOSITE_R, rr.COMPOSITE_LIVE   # 37 rays, 29 of them under a device-side count
SIGMA = dz.DEPTH_SIGMA


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device(DEV)


# ------------------------------------------------------------------------------------------------------------- kernel cases
_CASES = {}


def _case(R, S, dev):
    """Inputs on the host and the device and the float64 references, computed once per shape, shared by the tests and left unchanged."""
    key = (R, S)
    if key not in _CASES:
        inp = dz.depth_inputs(R, S, dz.depth_seed(S))
        d = {k: v.to(dev) for k, v in inp.items()}
        loss, loss_scale = dz.loss_ray_reference(inp)
        if R <= 64:
            g_ref, g_scale = dz.depth_backward_reference(inp)
        else:  # the big case: the closed form, which test_depth_cpu holds against the autograd reference, without a 160 K-row graph
            g_ref = dz.g_sigma_closed_form(inp)
            _, g_scale = dz.depth_backward_reference(inp)
        if len(_CASES) > 6:
            _CASES.clear()
        _CASES[key] = (inp, d, {"loss_ray": loss, "loss_scale": loss_scale, "g_sigma": g_ref, "g_scale": g_scale})
    return _CASES[key]


def _forward(case, R, S, n_dev=None, s=SIGMA):
    _, d, _ = case
    out = _poisoned({"loss_ray": torch.empty(R, device=d["sigma"].device)})["loss_ray"]
    check(_abi.load_library().rsn_depth_loss_forward(R, ptr(n_dev), S, ptr(d["eb"]), ptr(d["sigma"]), ptr(d["target"]), s, ptr(out),
                                                     ops._stream()))
    torch.cuda.synchronize()
    return out


def _backward(case, R, S, accumulate, n_dev=None, into=None, s=SIGMA):
    _, d, _ = case
    out = _poisoned({"g_sigma": torch.empty(R, S, device=d["sigma"].device)})["g_sigma"] if into is None else into
    check(_abi.load_library().rsn_depth_loss_backward(R, ptr(n_dev), S, ptr(d["eb"]), ptr(d["sigma"]), ptr(d["target"]), s,
                                                      ptr(d["g_loss_ray"]), ptr(out), accumulate, ops._stream()))
    torch.cuda.synchronize()
    return out


def _check(label, name, got, ref, scale, rows=None):
    got, ref, scale = got.detach().double().cpu(), ref.double(), scale.double()
    if rows is not None:
        got, ref, scale = got[:rows], ref[:rows], scale[:rows]
    assert bool(torch.isfinite(got).all()), f"{label} {name}: a value is not finite (not written, or the kernel produced it)"
    ratio = float(((got - ref).abs() / scale).max()) / EPS
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"RATIO {name} {ratio:.3f} [{label}] (bound {BOUND}, worst so far {WORST[name]:.3f})")
    assert ratio <= BOUND, f"{label} {name}: {ratio:.2f} x 2^-24 of the scale > {BOUND}"


def _is_poison(t):
    it, pattern = _POISON[t.dtype]
    return (t.view(it).reshape(t.shape[0], -1) == pattern).all(dim=1).cpu()


def _check_both(label, case, loss, g_sigma, rows=None):
    ref = case[2]
    _check(label, "loss_ray", loss, ref["loss_ray"], ref["loss_scale"], rows=rows)
    _check(label, "g_sigma", g_sigma, ref["g_sigma"], ref["g_scale"], rows=rows)


@pytest.mark.parametrize("S", S_CASES)
def test_forward_and_backward_match_fp64(dev, S):
    """Every ray is compared, the planted ones included; the ray without a target is held to exact zeros, and the empty ray to its
    closed form, -log(EPS) times the Gaussian mass of the bins."""
    case = _case(R_CASE, S, dev)
    inp = case[0]
    loss, gs = _forward(case, R_CASE, S), _backward(case, R_CASE, S, 0)
    _check_both(f"S{S}", case, loss, gs)
    none = (inp["target"] == 0).nonzero().flatten().tolist()
    assert dz.RAY_NO_TARGET in none and len(none) >= 2
    assert bool((loss[none] == 0).all()) and bool((gs[none] == 0).all()), "a ray without a target: loss and gradient are exactly 0"
    eb, D = inp["eb"][dz.RAY_EMPTY].double(), float(inp["target"][dz.RAY_EMPTY])
    s32 = float(np.float32(SIGMA))  # the float the ABI takes
    mass = float((torch.exp(-((eb[:-1] + eb[1:]) / 2 - D) ** 2 / (2 * s32 ** 2)) * (eb[1:] - eb[:-1])).sum())
    assert abs(float(loss[dz.RAY_EMPTY]) + math.log(dz.LOSS_EPS) * mass) <= 2 * EPS * 16.2 * mass


@pytest.mark.parametrize("S", (1, 65, 192))
def test_an_s_at_which_every_gaussian_underflows_gives_exact_zeros(dev, S):
    """s = 1e-20: exp(-(m - D)^2 / (2 s^2)) is 0 for every sample of every ray; loss and gradient are exactly 0 and finite, and the
    accumulate mode leaves the buffer's bits."""
    case = _case(R_CASE, S, dev)
    m = (case[0]["eb"][:, :-1].double() + case[0]["eb"][:, 1:].double()) / 2
    assert bool(((m - case[0]["target"].double()[:, None]).abs() > 1e-9).all()), "no midpoint may coincide with its target"
    loss, gs = _forward(case, R_CASE, S, s=dz.TINY_SIGMA), _backward(case, R_CASE, S, 0, s=dz.TINY_SIGMA)
    assert bool((loss == 0).all()) and bool((gs == 0).all())
    fill = (torch.rand(R_CASE, S, generator=torch.Generator().manual_seed(S)) - 0.5).to(dev)
    assert torch.equal(_backward(case, R_CASE, S, 1, into=fill.clone(), s=dz.TINY_SIGMA), fill)


@pytest.mark.parametrize("S", S_CASES)
def test_backward_accumulates_or_overwrites(dev, S):
    """accumulate = 1 onto a pre-filled g_sigma is pre-fill + the accumulate = 0 result, one fp32 rounding of the sum (torch's own fp32
    addition of the two: the same bits); accumulate = 0 leaves nothing of what the buffer held (it started poisoned)."""
    case = _case(R_CASE, S, dev)
    plain = _backward(case, R_CASE, S, 0)
    assert not bool(torch.isnan(plain).any()), "accumulate = 0 must overwrite every element"
    fill = (torch.rand(R_CASE, S, generator=torch.Generator().manual_seed(S)) - 0.5).to(dev)
    added = _backward(case, R_CASE, S, 1, into=fill.clone())
    assert torch.equal(added, fill + plain)
    assert not torch.equal(added, fill)


@pytest.mark.parametrize("S", (5, 130))
def test_device_side_count(dev, S):
    """29 of 37 rows: the rows under the count are written, the rows behind it are not touched."""
    case = _case(R_CASE, S, dev)
    n_dev = torch.tensor([LIVE], dtype=torch.int32, device=dev)
    loss, gs = _forward(case, R_CASE, S, n_dev), _backward(case, R_CASE, S, 0, n_dev)
    _check_both(f"count S{S}", case, loss, gs, rows=LIVE)
    assert bool(_is_poison(loss)[LIVE:].all()) and bool(_is_poison(gs)[LIVE:].all()), "rows behind the count were written"
    fill = (torch.rand(R_CASE, S, generator=torch.Generator().manual_seed(S + 1)) + 0.5).to(dev)
    added = _backward(case, R_CASE, S, 1, n_dev, into=fill.clone())
    assert torch.equal(added[LIVE:], fill[LIVE:]), "accumulate: rows behind the count were written"
    assert torch.equal(added[:LIVE], (fill + gs)[:LIVE])
    big = torch.tensor([R_CASE + 100], dtype=torch.int32, device=dev)  # a count above n_rays: n_rays holds
    assert torch.equal(_forward(case, R_CASE, S, big), _forward(case, R_CASE, S))


def test_grid_stride(dev):
    """32768 + 7 rays of 5 samples: the launch is capped at 8192 blocks of 4 rays, every wave walks a second ray and the last round is
    ragged."""
    R, S = rr.BIG_R, rr.BIG_S
    case = _case(R, S, dev)
    _check_both("grid stride", case, _forward(case, R, S), _backward(case, R, S, 0))


def test_repeatable_bits_and_the_sample_limit(dev):
    """No atomics and a fixed order of addition: two calls give the same bits.  S > 4096 is refused before a launch."""
    S = 130
    case = _case(R_CASE, S, dev)
    assert torch.equal(_forward(case, R_CASE, S), _forward(case, R_CASE, S))
    assert torch.equal(_backward(case, R_CASE, S, 0), _backward(case, R_CASE, S, 0))
    d = case[1]
    with pytest.raises(_abi.RsnError, match="n_samples=4097"):
        ops.depth_loss_forward(R_CASE, None, 4097, d["eb"], d["sigma"], d["target"], SIGMA)
    with pytest.raises(_abi.RsnError, match="n_samples=4097"):
        ops.depth_loss_backward(R_CASE, None, 4097, d["eb"], d["sigma"], d["target"], SIGMA, d["g_loss_ray"], d["sigma"])


# ------------------------------------------------------------------------------------------------------------- ray distances
GH, GW, GN = 37, 53, 3
GATHER_BOUND = 2.0 ** -23  # relative: one fp32 rounding (2^-24) plus the host's and the device's fp64 Newton solves' last bits


def _gather_inputs(table):
    rng = np.random.default_rng(11)
    depths = (0.5 + 4.0 * rng.random((GN, GH, GW))).astype(np.float32)
    depths[rng.random((GN, GH, GW)) < 0.15] = 0.0
    R = 700  # more than two blocks
    idx = np.stack([rng.integers(0, GN, R), rng.integers(0, GH, R), rng.integers(0, GW, R)], -1).astype(np.int32)
    idx[:4] = [(0, 0, 0), (GN - 1, GH - 1, GW - 1), (1, 0, GW - 1), (2, GH - 1, 0)]  # the corners: the largest radius
    level = (rng.random(R) < 0.3).astype(np.int32) * rng.integers(1, 3, R).astype(np.int32)
    cams = None if table is None else np.ascontiguousarray(table, dtype=np.float32)
    return depths, idx, level, cams


def _gather(depths, idx, level, cams, k, fisheye, euclidean, dev):
    t = ops.gather_ray_depth(torch.from_numpy(idx).to(dev), None if level is None else torch.from_numpy(level).to(dev),
                             torch.from_numpy(depths).to(dev), None if cams is None else torch.from_numpy(cams).to(dev), k, fisheye, euclidean)
    torch.cuda.synchronize()
    return t.cpu().double().numpy()


GATHER_TABLES = {
    "shared pinhole": None,
    "undistorted rows (9)": np.stack([cr.camera_row(GW, GH, coeffs=(0.0,) * 5, scale=1.0 + 0.1 * i) for i in range(GN)]),
    "distorted rows (9)": np.stack([cr.camera_row(GW, GH, scale=1.0 + 0.1 * i) for i in range(GN)]),
    "distorted rows (12)": np.stack([lr.perspective_row12(GW, GH, scale=1.0 + 0.1 * i) for i in range(GN)]),
}


@pytest.mark.parametrize("name", list(GATHER_TABLES))
@pytest.mark.parametrize("with_levels", [False, True])
def test_gather_ray_depth_matches_the_fp64_restatement(dev, name, with_levels):
    """z-depths through the shared pinhole, an undistorted and a distorted 9-column table and a 12-column one: within 2^-23 relative of
    float64; a stored 0 and a ray of a level above 0 give exact 0; euclidean maps come back bit for bit."""
    depths, idx, level, cams = _gather_inputs(GATHER_TABLES[name])
    level = level if with_levels else None
    k = (61.0, 64.5, GW / 2 - 0.7, GH / 2 + 0.4)
    got = _gather(depths, idx, level, cams, k, False, False, dev)
    want = dz.ray_depth_reference(idx, level, depths, cams, k, False)
    zero = want == 0.0
    assert zero.sum() >= 50 and (~zero).sum() >= 300 and np.all(got[zero] == 0.0)
    if with_levels:
        assert np.all(got[level > 0] == 0.0) and (level > 0).sum() >= 100
    rel = np.abs(got - want)[~zero] / want[~zero]
    print(f"RATIO gather [{name}, levels {with_levels}]: worst {rel.max() / 2.0 ** -24:.3f} x 2^-24 (bound 2)")
    assert rel.max() <= GATHER_BOUND
    stored = depths[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float64)
    assert np.all(want[~zero] >= stored[~zero])  # |v| >= 1: a distance along the ray is never below the z-depth
    eu = _gather(depths, idx, level, cams, k, False, True, dev)
    assert np.array_equal(eu, np.where(level > 0, 0.0, stored) if with_levels else stored)


def test_gather_ray_depth_on_fisheye_rows(dev):
    """A 12-column table with fisheye rows: euclidean maps are served as stored; z-depths are refused on the host, without a launch
    (the output stays poisoned), and through the data manager at construction."""
    table = np.stack([lr.fisheye_row(GW, GH), lr.perspective_row12(GW, GH), lr.fisheye_row(GW, GH, corner_theta_d=2.0)])
    depths, idx, level, cams = _gather_inputs(table)
    stored = depths[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float64)
    assert np.array_equal(_gather(depths, idx, None, cams, None, True, True, dev), stored)
    with pytest.raises(_abi.RsnError, match="fisheye"):
        _gather(depths, idx, None, cams, None, True, False, dev)
    t = _poisoned({"t": torch.empty(len(idx), device=dev)})["t"]
    d_idx, d_depths, d_cams = torch.from_numpy(idx).to(dev), torch.from_numpy(depths).to(dev), torch.from_numpy(cams).to(dev)
    rc = _abi.load_library().rsn_gather_ray_depth(len(idx), ptr(d_idx), None, ptr(d_depths), GN, GH, GW, ptr(d_cams), 12, 0.0, 0.0, 0.0, 0.0,
                                                  1, 0, ptr(t), ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and bool(_is_poison(t.view(-1, 1)).all()), "the refusal must come before any launch"
    scene = BlenderScene.from_arrays(np.zeros((GN, GH, GW, 3), np.uint8), cr.shell_poses(GN), focal=60.0, depths=depths)
    scene.cameras = cams
    with pytest.raises(ValueError, match="depth_euclidean"):
        RayDataManager(scene, dev)
    dm = RayDataManager(scene, dev, num_rays_per_batch=64, depth_euclidean=True)
    rb, batch = dm.next_train(0)
    i = batch["indices"].cpu().numpy()
    assert np.array_equal(batch["depth"].cpu().numpy(), depths[i[:, 0], i[:, 1], i[:, 2]])
    assert torch.equal(rb.metadata["depth"], batch["depth"].view(-1, 1))


def test_data_manager_serves_depths_without_a_host_read(dev):
    """next_train on a scene with depth maps: batch["depth"] is the float64 restatement of the batch's own indices (levels > 1: the
    rays of a level above 0 get no target), no device-to-host read; the same scene without depths draws the same rays and has no
    such key."""
    rng = np.random.default_rng(2)
    depths = (1.0 + rng.random((GN, 32, 48))).astype(np.float32)
    depths[:, :4] = 0.0
    ims = rng.integers(0, 255, (GN, 32, 48, 3)).astype(np.uint8)
    scene = BlenderScene.from_arrays(ims, cr.shell_poses(GN), focal=50.0, depths=depths)
    plain = BlenderScene.from_arrays(ims, cr.shell_poses(GN), focal=50.0)
    for levels in (1, 3):
        dm, dm0 = RayDataManager(scene, dev, num_rays_per_batch=512, seed=3, levels=levels), RayDataManager(plain, dev, 512, seed=3, levels=levels)
        dm.next_train(0)  # warm-up
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            rb, batch = dm.next_train(7)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        rb0, batch0 = dm0.next_train(7)
        assert "depth" not in batch0 and rb0.metadata is None and set(batch) == set(batch0) | {"depth"}
        assert torch.equal(rb.origins, rb0.origins) and torch.equal(batch["image"], batch0["image"]) and torch.equal(batch["indices"], batch0["indices"])
        lv = batch["levels"].cpu().numpy() if levels > 1 else None
        want = dz.ray_depth_reference(batch["indices"].cpu().numpy(), lv, depths, None, (50.0, 50.0, 24.0, 16.0), False)
        got = batch["depth"].cpu().double().numpy()
        assert np.all(got[want == 0] == 0) and np.abs(got - want).max() <= GATHER_BOUND * want.max()
        if levels > 1:
            assert (lv > 0).sum() > 100 and np.all(got[lv > 0] == 0) and (got > 0).sum() > 50
    assert torch.equal(dm.depth_image(1), torch.from_numpy(depths[1]).to(dev))
    view = dm.view_ray_depth(2).cpu().double().numpy()
    yy, xx = np.meshgrid(np.arange(32), np.arange(48), indexing="ij")
    idx = np.stack([np.full_like(yy, 2), yy, xx], -1).reshape(-1, 3)
    want = dz.ray_depth_reference(idx, None, depths, None, (50.0, 50.0, 24.0, 16.0), False).reshape(32, 48)
    assert np.abs(view - want).max() <= GATHER_BOUND * want.max() and np.all(view[:4] == 0)
    with pytest.raises(ValueError, match="no depth maps"):
        dm0.depth_image(0)


# ------------------------------------------------------------------------------------------------------------- eval metric
def test_depth_error_matches_fp64(dev):
    """A 33 x 17 view (three workgroups, a ragged last one) with invalid pixels and a mask: both sums within 2^-24 of themselves (every
    term is non-negative: the sum is its own scale; fp64 inside, one fp32 rounding), the count exact; the same without the mask; and
    metrics.depth_error's figures without a device-to-host read."""
    H, W = 33, 17
    g = torch.Generator().manual_seed(4)
    depth = 2.0 + 3.0 * torch.rand(H, W, generator=g)
    target = (depth + 0.3 * (torch.rand(H, W, generator=g) - 0.5)) * (torch.rand(H, W, generator=g) > 0.25)
    mask = (torch.rand(H, W, generator=g) > 0.3).to(torch.uint8)
    lib = _abi.load_library()
    nbytes = int(lib.rsn_normal_error_workspace_bytes(H * W))
    for m in (mask, None):
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        out = _poisoned({"out": torch.empty(3, device=dev)})["out"]
        d, t, md = depth.to(dev), target.to(dev), None if m is None else m.to(dev)
        check(lib.rsn_depth_error(H * W, ptr(d), ptr(t), ptr(md), ptr(ws), nbytes, ptr(out), ops._stream()))
        torch.cuda.synchronize()
        a, b, n = dz.depth_error_reference(depth.numpy(), target.numpy(), None if m is None else m.numpy())
        got = out.cpu().double().tolist()
        print(f"RATIO depth_error mask {m is not None}: abs {abs(got[0] - a) / a / EPS:.3f}, sq {abs(got[1] - b) / b / EPS:.3f} x 2^-24; count {got[2]:.0f} of {H * W}")
        assert abs(got[0] - a) <= EPS * a and abs(got[1] - b) <= EPS * b and got[2] == n and 100 < n < H * W
        again = torch.empty(3, device=dev)
        check(lib.rsn_depth_error(H * W, ptr(d), ptr(t), ptr(md), ptr(ws), nbytes, ptr(again), ops._stream()))
        assert torch.equal(again, out), "a fixed order of addition: the same bits"
    d3, mb = depth.to(dev).view(H, W, 1), mask.to(dev).bool()
    metrics.depth_error(d3, t, mb)  # warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = metrics.depth_error(d3, t, mb)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    a, b, n = dz.depth_error_reference(depth.numpy(), target.numpy(), mask.numpy())
    assert float(res["depth_mae"]) == pytest.approx(a / n, rel=1e-6) and float(res["depth_rmse"]) == pytest.approx(math.sqrt(b / n), rel=1e-6)
    assert float(res["depth_pixels"]) == n and float(res["depth_valid"]) == pytest.approx(n / (H * W), rel=1e-6)
    none = metrics.depth_error(depth.to(dev), torch.zeros(H, W, device=dev))
    assert math.isnan(float(none["depth_mae"])) and float(none["depth_pixels"]) == 0.0
    for bad in (lambda: metrics.depth_error(depth, target), lambda: metrics.depth_error(depth.to(dev), target.to(dev)[:-1]),
                lambda: metrics.depth_error(depth.to(dev).double(), target.to(dev)), lambda: metrics.depth_error(depth.to(dev), target.to(dev), mask.to(dev).float())):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------------------- the whole step
LAMBDA = 0.01  # weight of the depth term in the oracle comparison; the test asserts that it matters at this size
STEP_SIGMA = 0.3


def _depth_mean(eb, sigma, target, s):
    """mean over the rays of the reference formula in float64, differentiable in the oracle's fp32 sigma [R,S,1] (sigma.double())."""
    w, _, _, k = dz._terms({"eb": eb, "target": target}, s, sigma[..., 0].double(), None)
    return (-torch.log(w + dz.LOSS_EPS) * k).sum(-1).mean()


def _oracle_sigma(P, fs, rays, eb, detached_weights, mean):
    """The oracle's own sigma of a level once more, attached to the parameters (cpu_ref.get_outputs hands its weights out detached):
    field_level on the same bins and contracted means; its weights are what the oracle returned, bit for bit."""
    lv = cpu_ref.field_level(P, fs, *rays, eb, True, want_normals=False, mean_override=mean)
    assert torch.equal(cpu_ref.weights_from_density(lv["sigma"], lv["t0"], lv["t1"]).detach(), detached_weights)
    return lv["sigma"]


def _density_head(grads):
    return torch.cat([grads["field_output_density.net.weight"].flatten(), grads["field_output_density.net.bias"].flatten()]).double()


@pytest.mark.parametrize("mma", ["f32", "bf16x6"])
def test_train_step_with_the_term_matches_oracle_autograd(dev, mma):
    """The 4 x 64 field with both depth terms on, on identical sample positions (the method of test_distortion_gpu's part (b)): the
    reference side takes the oracle's sigma, forms the weights and the term in float64 inside the autograd graph and continues through
    the unchanged fp32 oracle (an fp32 1 / (w + EPS) there would make the reference the noisier party).  Every parameter gradient
    within 5e-5 of the tensor's largest entry, the distortion step test's bound.  In the oracle the term must carry at least a tenth
    of the gradient norm of the density head, or this shows nothing."""
    layers, width, samples, R, bias = 4, 64, (16, 16, 8, 8), 40, 2.0
    seed = layers * 7 + width
    torch.manual_seed(seed)
    cfg = pkg.ReflectSamplingNeRFModelConfig(
        num_coarse_samples=samples[0], num_importance_samples=samples[1], num_reflect_coarse_samples=samples[2],
        num_reflect_importance_samples=samples[3], base_mlp_num_layers=layers, base_mlp_layer_width=width)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += bias
    P = {k: v.detach().clone().requires_grad_(True) for k, v in model.field.state_dict().items()}
    model.to(dev).train()
    model.field.set_mma_mode(mma)
    model.depth_sigma = STEP_SIGMA
    model.config.loss_coefficients.update(depth_loss_coarse=LAMBDA, depth_loss_fine=LAMBDA)
    o, d, pa = cpu_ref.synthetic_rays(R, seed=seed + 50)
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    fs, ms = cpu_ref.FieldSpec(num_layers=layers, width=width), cpu_ref.ModelSpec(*samples)
    g = torch.Generator().manual_seed(seed + 1)
    jit = {"coarse": torch.rand(R, samples[0] + 1, generator=g), "fine": torch.rand(R, samples[1] + 1, generator=g),
           "reflect_coarse": torch.rand(R, samples[2] + 1, generator=g), "reflect_fine": torch.rand(R, samples[3] + 1, generator=g)}
    tgt = {k: torch.rand(R, 3, generator=g) for k in ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine")}
    target = (2.5 + 3.0 * torch.rand(R, generator=g)) * (torch.rand(R, generator=g) > 0.2)
    assert 0 < int((target == 0).sum()) < R // 2
    tgt_dev = {k: v.to(dev) for k, v in tgt.items()}
    rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev), nears=nears.to(dev), fars=fars.to(dev),
                       metadata={"depth": target.view(R, 1).to(dev)})

    def oracle_grads():
        out = {k: p.grad.clone() for k, p in P.items() if p.grad is not None}
        for p in P.values():
            p.grad = None
        return out

    ref = cpu_ref.get_outputs(P, fs, ms, o, d, pa, nears, fars, training=True, jitter=jit)
    assert int(ref["mask"].sum()) > 0
    jit_gpu = dict(jit, reflect_coarse=jit["reflect_coarse"][ref["mask"]], reflect_fine=jit["reflect_fine"][ref["mask"]])
    model.zero_grad(set_to_none=True)
    model._keep_train_state = True
    out = model._get_outputs_train(rb, jitter=jit_gpu)
    st = model._train_state
    model._keep_train_state, model._train_state = False, None
    assert tuple(out.fused) == train_graph.FUSED_KEYS + train_graph.DEPTH_KEYS
    assert torch.equal(out["mask"].cpu(), ref["mask"])
    M = int(ref["mask"].sum())
    hip_bins, hip_means = {}, {}
    for name, sbk, ebk, lvk, n, S in (("coarse", "sb_c", "eb_c", "lc", R, samples[0]), ("fine", "sb_f", "eb_f", "lf", R, samples[1]),
                                      ("reflect_coarse", "sb_rc", "eb_rc", "lrc", M, samples[2]),
                                      ("reflect_fine", "sb_rf", "eb_rf", "lrf", M, samples[3])):
        hip_bins[name + "_spacing"], hip_bins[name + "_euclid"] = st[sbk].cpu(), st[ebk].cpu()
        hip_means[name] = st[lvk]["saved"]["enc"][:, 96:99].reshape(n, S, 3).cpu()
    ref2 = cpu_ref.get_outputs(P, fs, ms, o, d, pa, nears, fars, training=True, jitter=jit, bins=hip_bins, means=hip_means)
    _loss_from_outputs(ref2, tgt).backward(retain_graph=True)
    g_plain = oracle_grads()
    sig_c = _oracle_sigma(P, fs, (o, d, pa), hip_bins["coarse_euclid"], ref2["weights_coarse"], hip_means["coarse"])
    sig_f = _oracle_sigma(P, fs, (o, d, pa), hip_bins["fine_euclid"], ref2["weights_fine"], hip_means["fine"])
    term_c = _depth_mean(hip_bins["coarse_euclid"], sig_c, target, STEP_SIGMA)
    term_f = _depth_mean(hip_bins["fine_euclid"], sig_f, target, STEP_SIGMA)
    (_loss_from_outputs(ref2, tgt).double() + LAMBDA * (term_c + term_f)).backward()
    g_ref = oracle_grads()
    share = float((_density_head(g_ref) - _density_head(g_plain)).norm() / _density_head(g_ref).norm())
    print(f"depth term's share of the density head's gradient norm in the oracle: {share:.3f}")
    assert share >= 0.1, f"LAMBDA = {LAMBDA}: the depth term is {share:.3f} of the density head's gradient; the comparison shows nothing"
    for key, term in (("depth_loss_ray_coarse", term_c), ("depth_loss_ray_fine", term_f)):
        got, want = float(out.fused[key].detach().double().mean()), float(term)
        assert abs(got - want) <= 1e-4 * abs(want), (key, got, want)  # the HIP side's sigma is its own fp32 evaluation of the field
        assert bool((out.fused[key][(target == 0).to(dev)] == 0).all())
    checked = dict(out)
    checked["normals_coarse"] = ref2["normals_coarse"].detach().to(dev)
    checked["normals_fine"] = ref2["normals_fine"].detach().to(dev)
    (_loss_from_outputs(checked, tgt_dev) + LAMBDA * (out.fused["depth_loss_ray_coarse"].mean()
                                                      + out.fused["depth_loss_ray_fine"].mean())).backward()
    torch.cuda.synchronize()
    worst = (0.0, "")
    for name, p in model.field.named_parameters():
        if "field_output_low" in name:
            assert p.grad is None and name not in g_ref
            continue
        gr = g_ref[name]
        worst = max(worst, (float((p.grad.cpu() - gr).abs().max()) / float(gr.abs().max()), name))
    print(f"identical positions, full loss + both depth terms ({mma}): worst gradient error / tensor max {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 5e-5, f"identical positions: {worst[1]} off by {worst[0]:.3e} of its largest entry"


def _with_target(rb, R, dev, seed=9):
    g = torch.Generator().manual_seed(seed)
    t = (2.5 + 3.0 * torch.rand(R, generator=g)) * (torch.rand(R, generator=g) > 0.2)
    rb.metadata = {"depth": t.view(R, 1).to(dev)}
    return rb


def test_loss_dict_keys_and_the_off_path_bits(dev):
    """Absent and 0.0 coefficients, with and without a target on the rays: exactly the eight reference keys, outputs.fused holds
    FUSED_KEYS only, and under the deterministic mode the parameter gradients of all of them are the same bits.  Both set: ten keys,
    device tensors, coef * mean; set without a target: refused."""
    model, rb, batch = _train_setup(dev, 64, (16, 16, 8, 8), layers=4, width=64)
    model.set_deterministic(True)
    coef = model.config.loss_coefficients
    grads = []
    for zeros, targets in ((False, False), (True, False), (False, True), (True, True)):
        coef.pop("depth_loss_coarse", None), coef.pop("depth_loss_fine", None)
        if zeros:
            coef.update(depth_loss_coarse=0.0, depth_loss_fine=0.0)
        rb.metadata = None
        if targets:
            _with_target(rb, 64, dev)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        out = model(rb)
        assert set(out.fused) == set(train_graph.FUSED_KEYS)
        ld = model.get_loss_dict(out, batch)
        assert tuple(ld) == train_ops.LOSS_TERMS
        sum(ld.values()).backward()
        grads.append({n: p.grad.clone() for n, p in model.field.named_parameters() if p.grad is not None})
    for other in grads[1:]:
        assert sorted(grads[0]) == sorted(other) and all(torch.equal(grads[0][n], other[n]) for n in other)
    coef.update(depth_loss_coarse=0.5, depth_loss_fine=0.25)
    torch.manual_seed(5)
    out = model(rb)
    assert tuple(out.fused) == train_graph.FUSED_KEYS + train_graph.DEPTH_KEYS
    ld = model.get_loss_dict(out, batch)
    assert tuple(ld) == train_ops.LOSS_TERMS + ("depth_loss_coarse", "depth_loss_fine") and len(ld) == 10
    for key, ray_key, c in (("depth_loss_coarse", "depth_loss_ray_coarse", 0.5), ("depth_loss_fine", "depth_loss_ray_fine", 0.25)):
        assert ld[key].is_cuda and ld[key].dim() == 0 and ld[key].requires_grad
        want = c * float(out.fused[ray_key].detach().double().mean())
        assert abs(float(ld[key].detach()) - want) <= 1e-6 * abs(want) and want != 0
    coef.update(distortion_loss_fine=0.01)  # beside the distortion term: its outputs come first
    out = model(rb)
    assert tuple(out.fused) == train_graph.FUSED_KEYS + ("dist_loss_ray_fine",) + train_graph.DEPTH_KEYS
    sum(model.get_loss_dict(out, batch).values()).backward()
    coef.pop("distortion_loss_fine")
    rb.metadata = None
    with pytest.raises(_abi.RsnError, match="carry no target"):
        model(rb)
    assert model._depth_target is None


def test_the_term_reaches_the_density_head(dev):
    """What the term adds to the density head's gradient (on minus off, same jitter) points where the float64 reference's g_sigma,
    pushed through the same saved sigma, says: the HIP g_sigma of both levels against depth_reference on the step's own sigma and
    bins, cosine above 0.99 (it is the same fp64 formula on the same fp32 inputs: the bound of the kernel tests holds here too)."""
    R, samples = 64, (16, 16, 8, 8)
    model, rb, batch = _train_setup(dev, R, samples, layers=4, width=64)
    _with_target(rb, R, dev)
    model.config.loss_coefficients.update(depth_loss_coarse=1.0, depth_loss_fine=1.0)
    model.depth_sigma = STEP_SIGMA
    model._keep_train_state = True
    model(rb)
    st = model._train_state
    model._keep_train_state, model._train_state = False, None
    for lvk, ebk, S in (("lc", "eb_c", samples[0]), ("lf", "eb_f", samples[1])):
        inp = {"sigma": st[lvk]["sigma"].reshape(R, S).cpu(), "eb": st[ebk].cpu(), "target": rb.metadata["depth"].flatten().cpu(),
               "g_loss_ray": torch.full((R,), 1.0 / R)}
        g_sigma = torch.zeros(R, S, device=dev)
        ops.depth_loss_backward(R, None, S, st[ebk], st[lvk]["sigma"], rb.metadata["depth"].flatten().contiguous(), STEP_SIGMA,
                                inp["g_loss_ray"].to(dev), g_sigma, accumulate=True)
        ref, scale = dz.depth_backward_reference(inp, s=STEP_SIGMA)
        got = g_sigma.cpu().double()
        cos = float((got * ref).sum() / (got.norm() * ref.norm()))
        print(f"{lvk}: g_sigma against float64, cosine {cos:.9f}, worst ratio {float(((got - ref).abs() / scale).max()) / EPS:.3f} x 2^-24")
        assert cos > 0.99 and float(((got - ref).abs() / scale).max()) <= dz.BOUND
    grads = {}
    for on in (False, True):
        model.config.loss_coefficients.update(depth_loss_coarse=float(on), depth_loss_fine=float(on))
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        sum(model.get_loss_dict(model(rb), batch).values()).backward()
        grads[on] = _density_head({n: p.grad.detach().cpu() for n, p in model.field.named_parameters() if p.grad is not None})
    added = grads[True] - grads[False]
    assert float(added.norm()) > 0.1 * float(grads[True].norm()), "the term does not reach the density head"


def test_chunked_train_step_equals_whole_batch_step_with_the_term(dev):
    """test_gpu_parity.test_chunked_train_step_equals_whole_batch_step with both depth terms on, at its bounds: the terms are means
    over the rays (parallel._MEAN_TERMS), and the targets are sliced with the rays."""
    from reflect_sampling_nerf_amd.parallel import train_step

    R = 320
    real_rand = torch.rand
    results = []
    try:
        torch.rand = lambda *shape, **kw: torch.full(shape, 0.37, **{k: v for k, v in kw.items() if k in ("device", "dtype")})
        for chunk in (None, 96):
            torch.manual_seed(0)
            cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=16, num_importance_samples=24,
                                                    num_reflect_coarse_samples=8, num_reflect_importance_samples=8,
                                                    base_mlp_num_layers=8, base_mlp_layer_width=64)
            model = cfg.setup(scene_box=None, num_train_data=1)
            with torch.no_grad():
                model.field.field_output_density.net.bias += 2.0
            model.to(dev).train()
            model.config.loss_coefficients.update(depth_loss_coarse=0.005, depth_loss_fine=0.01)
            model.depth_sigma = STEP_SIGMA
            o, d, pa = cpu_ref.synthetic_rays(R, seed=3)
            rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev),
                               nears=torch.full((R, 1), 2.0, device=dev), fars=torch.full((R, 1), 6.0, device=dev))
            g = real_rand(R, 2, generator=torch.Generator().manual_seed(9))
            rb.metadata = {"depth": ((2.5 + 3.0 * g[:, :1]) * (g[:, 1:] > 0.2)).to(dev)}
            batch = {"image": real_rand(R, 3, generator=torch.Generator().manual_seed(1)).to(dev)}
            params = model.get_param_groups()["fields"]
            opt = pkg.FusedRAdam(params, lr=1e-3, eps=1e-15)
            loss = float(train_step(model, rb, batch, opt, None, 100, ray_chunk=chunk))
            torch.cuda.synchronize()
            results.append((loss, {n: p.grad.clone() for n, p in model.field.named_parameters() if p.grad is not None},
                            [p.detach().clone() for p in params]))
    finally:
        torch.rand = real_rand
    (l0, g0, p0), (l1, g1, p1) = results
    assert abs(l0 - l1) <= 1e-5 * abs(l0)
    assert sorted(g0) == sorted(g1)
    for n in g0:
        scale = float(g0[n].abs().max())
        assert float((g0[n] - g1[n]).abs().max()) <= 2e-5 * scale + 1e-10, n
    for a, b in zip(p0, p1):
        assert float((a - b).abs().max()) <= 1e-6


def test_training_step_with_the_term_issues_no_device_to_host_read(dev):
    """The method of test_gpu_parity.test_training_step_issues_no_device_to_host_read, with both depth terms on."""
    from reflect_sampling_nerf_amd.parallel import train_step

    model, rb, batch = _train_setup(dev, 192, (24, 24, 16, 16))
    _with_target(rb, 192, dev)
    model.config.loss_coefficients.update(depth_loss_coarse=0.002, depth_loss_fine=0.01)
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    train_step(model, rb, batch, opt, None, 100)  # warm-up: one-time uploads
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for k in range(3):
            loss = train_step(model, rb, batch, opt, None, 101 + k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(loss))


# ------------------------------------------------------------------------------------------------------------- trainer
X = 0.01
SPHERE_RADIUS = 0.8


def depth_sphere_scene(n, H=48, W=48, offset=0.0):
    """The Lambert sphere of the tests (radius 0.8, white background) seen from a radius-4 shell, with analytic depth maps: the
    ray-sphere distance t along the normalised ray, converted to the z-depth t / |(X, -Y, -1)| that phone captures store; 0 off the
    sphere (no measurement)."""
    poses = cr.shell_poses(n, offset=offset)
    focal = 0.5 * W / math.tan(0.5 * 0.6911112070083618)
    row = np.array([focal, focal, W / 2, H / 2, 0, 0, 0, 0, 0], np.float64)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ims, depths = [], []
    for p in poses:
        ims.append(cr.sphere_image(p, row, H, W, SPHERE_RADIUS))
        o, d, _ = cr.rays(p, row, yy, xx)
        b = (o * d).sum(-1)
        disc = b * b - ((o * o).sum(-1) - SPHERE_RADIUS ** 2)
        t = -b - np.sqrt(np.clip(disc, 0, None))
        norm = np.sqrt(((xx + 0.5 - W / 2) / focal) ** 2 + ((yy + 0.5 - H / 2) / focal) ** 2 + 1.0)
        depths.append(np.where(disc > 0, t / norm, 0.0))
    return BlenderScene.from_arrays(np.stack(ims), poses.astype(np.float32), focal=focal, depths=np.stack(depths))


@pytest.fixture(scope="module")
def scene():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return depth_sphere_scene(6)


@pytest.fixture(scope="module")
def run_six(scene, tmp_path_factory):
    """6 deterministic steps with depth_loss X and a depth_sigma of its own (checkpoints at steps 3 and 5): trained once, read by both
    trainer tests."""
    return _Run(scene, tmp_path_factory.mktemp("depth_a"), steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True,
                depth_loss=X, depth_sigma=0.2)


def test_trainer_runs_are_bit_reproducible_with_the_term(scene, run_six, tmp_path):
    """Two deterministic runs of 6 steps with the term: identical parameters and moments.  The run records what was set, its first
    log line names it, and it differs from the run without the term -- which records nothing, and which is, bit for bit, the run on
    the same scene without depth maps."""
    again = _Run(scene, tmp_path / "b", steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True, depth_loss=X, depth_sigma=0.2)
    assert _differing(run_six.ckpt(5), again.ckpt(5)) == []
    rs = _load(run_six.ckpt(5))["rsn_run"]
    assert rs["depth_loss"] == X and rs["depth_sigma"] == 0.2 and "depth_loss_coarse" not in rs and "depth_euclidean" not in rs and rs["version"] == 1
    assert "depth_loss_fine 0.01" in run_six.logs[0] and "depth_sigma 0.2" in run_six.logs[0] and "depth_loss_coarse" not in run_six.logs[0]
    plain = _Run(scene, tmp_path / "c", steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True)
    assert "depth" not in plain.logs[0] and not any(k.startswith("depth") for k in _load(plain.ckpt(5))["rsn_run"])
    assert any(k.startswith("pipeline/") for k in _differing(run_six.ckpt(5), plain.ckpt(5))), "the term changed nothing"
    import dataclasses

    bare = _Run(dataclasses.replace(scene, depths=None), tmp_path / "e", steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True)
    assert _differing(plain.ckpt(5), bare.ckpt(5)) == [] and all(torch.equal(plain.losses[s], bare.losses[s]) for s in range(6))
    with pytest.raises(ValueError, match="no depth maps"):
        _Run(dataclasses.replace(scene, depths=None), tmp_path / "f", steps=2, save_every=0, rays=96, depth_loss=X)


def test_trainer_resume_restores_the_settings_bit_exactly(scene, run_six, tmp_path):
    """3 steps, then resume to 6 WITHOUT the arguments: coefficient and sigma come from the checkpoint and the result is the
    uninterrupted run's."""
    first = _Run(scene, tmp_path / "d", steps=3, save_every=0, rays=96, mma="f32", seed=0, deterministic=True, depth_loss=X, depth_sigma=0.2)
    assert first.saved_steps() == [2]
    rest = _Run(scene, tmp_path / "d", steps=6, save_every=3, resume=first.ckpt(2))
    assert "depth_loss_fine 0.01" in rest.logs[0] and "depth_sigma 0.2" in rest.logs[0]
    assert _differing(run_six.ckpt(5), rest.ckpt(5)) == []
    assert all(torch.equal(run_six.losses[s], rest.losses[s]) for s in (3, 4, 5))
    rs = _load(rest.ckpt(5))["rsn_run"]
    assert rs["depth_loss"] == X and rs["depth_sigma"] == 0.2


# ------------------------------------------------------------------------------------------------------------- end to end
E2E_STEPS = 800     # 400, where the other toy tests sit, separates no arm: depth_fine is the median depth, which stays at the far end of
                    # a ray until its accumulation passes one half (measured at 400 steps: 2.143 without, 2.134 to 2.157 with)
E2E_COEF = 10.0     # the test's own: a coefficient at which 800 toy steps separate the arms; not a recommendation
E2E_SIGMA = 0.1
# This test's own deterministic runs on an MI355X (profiles/depth_loss.json, "toy_scene"): held-out depth_rmse after E2E_STEPS steps
# without the term (the parent's behaviour) and with it.  The test asks for half the measured reduction, as the lens test does with
# its PSNR gain.
# Measured: 2.3596 -> 0.5117 (coefficient 1: 1.9602; sigma 0.3, coefficient 1: 0.7239; after 1600 steps 2.3106 -> 0.2635).
E2E_MEASURED_RMSE = {"off": 2.3596, "on": 0.5117}


def _e2e_cfg():
    return pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=32, num_importance_samples=32, num_reflect_coarse_samples=16,
                                             num_reflect_importance_samples=16, base_mlp_num_layers=4, base_mlp_layer_width=64)


def run_end_to_end(out_dir, steps=E2E_STEPS, coef=E2E_COEF, sigma=E2E_SIGMA, arms=("off", "on")):
    """train (deterministic) with and without the term on 24 views -> eval --depth on 4 held-out views; -> {arm: results}."""
    import os

    train_scene, test_scene = depth_sphere_scene(24), depth_sphere_scene(4, offset=0.37)
    kw = dict(steps=steps, rays=1024, save_every=0, log_every=0, seed=0, device=DEV, log=None, deterministic=True, model_config=_e2e_cfg())
    out = {}
    for arm in arms:
        extra = dict(depth_loss=coef, depth_sigma=sigma) if arm == "on" else {}
        ck = trainer.train(train_scene, os.path.join(str(out_dir), arm), **kw, **extra)
        res = trainer.evaluate(test_scene, ck, device=DEV, model_config=_e2e_cfg(), depth=True)
        r = res["results"]
        assert {"depth_mae", "depth_mae_std", "depth_rmse", "depth_rmse_std", "depth_valid"} <= set(r) and "depth" in res
        assert all({"depth_mae", "depth_rmse", "depth_valid"} <= set(p) for p in res["per_image"]) and len(res["per_image"]) == 4
        assert 0.05 < r["depth_valid"] < 0.5 and r["depth_mae"] <= r["depth_rmse"]
        out[arm] = {k: r[k] for k in ("depth_mae", "depth_rmse", "depth_valid", "psnr", "fine_psnr")}
        if arm == "off":  # without --depth the JSON is what it always was
            base = trainer.evaluate(test_scene, ck, device=DEV, model_config=_e2e_cfg(), max_images=1)
            assert not any(k.startswith("depth") for k in base["results"]) and "depth" not in base
            assert not any(k.startswith("depth") for k in base["per_image"][0])
            with_d = {k: v for k, v in res["per_image"][0].items() if not k.startswith("depth") and k not in ("num_rays_per_sec", "fps")}
            assert with_d == {k: v for k, v in base["per_image"][0].items() if k not in ("num_rays_per_sec", "fps")}
    return out


def test_depth_supervision_end_to_end_on_the_sphere(tmp_path):
    numbers = run_end_to_end(tmp_path)
    off, on = numbers["off"]["depth_rmse"], numbers["on"]["depth_rmse"]
    print(f"depth end to end: held-out depth_rmse {off:.4f} without the term -> {on:.4f} with it ({E2E_STEPS} steps, coefficient {E2E_COEF}, "
          f"sigma {E2E_SIGMA}); measured {E2E_MEASURED_RMSE}; psnr {numbers['off']['psnr']:.2f} -> {numbers['on']['psnr']:.2f}")
    bound = 0.5 * (E2E_MEASURED_RMSE["off"] - E2E_MEASURED_RMSE["on"])
    assert bound > 0 and off - on >= bound, numbers
