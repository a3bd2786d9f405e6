"""The distortion loss (mip-NeRF 360 eq. 15) on the GPU: rsn_distortion_forward / rsn_distortion_backward called directly through the C
ABI against the float64 references of tests/distortion_reference.py at the shapes where the kernels change path (one lane, a full
wave +- 1, ragged 64-sample chunks, the grid-stride ray loop, a device-side count), then the term inside the whole training step
against autograd through the oracle, the loss dictionary, parallel.train_step and the trainer.
Every output buffer starts as tests.helpers._POISON."""
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, ops, train_graph, train_ops
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import distortion_reference as dr
from tests import render_reference as rr
from tests.helpers import _POISON, _poisoned
from tests.test_gpu_parity import _coarse_loss, _loss_from_outputs, _train_setup
from tests.test_resume_gpu import _differing, _load, _Run, _sphere_scene

pytestmark = pytest.mark.gpu

EPS = rr.EPS
# |got - fp64 reference| / scale in units of 2^-24, the convention of test_render_ops_gpu.py: the scale is the fp64 sum of the absolute
# values of the terms the output adds (loss_ray: the value itself, every term being non-negative; g_sigma:
# delta_k (|g_w[k]| T_{k+1} + sum_{i>k} |g_w[i]| w_i), distortion_reference.distortion_backward_reference).  The allowance for fp32's
# rounding of the optical depth that test_render_ops_gpu._check_sum grants is not taken: neither kernel evaluates exp(-X) in fp32 (the
# forward is compared on the very weights it read, the backward derives its own in fp64).  Worst ratio measured on MI355X over all
# cases of this file (the RATIO lines these tests print), and the bound at 4x that.  CEILING is derived, not measured: a few fp32
# roundings and one expf per term, the scans in fp64.  A measured ratio whose 4x exceeds it is a kernel defect: the backward first read
# rsn_composite's fp32 weights and measured 4388 x 2^-24 on a ray whose only sample has sigma = 1.4e-4 (those weights are good to
# 2^-24 of the transmittance, not of the weight), which is why it now re-derives them.
CEILING = 64 * EPS
BOUNDS = {  # name: (measured / 2^-24, bound / 2^-24)
    "loss_ray": (0.990, 3.96),  # the fp64 sum rounded to fp32 once
    "g_sigma": (0.998, 3.99),   # likewise
}
assert all(4 * m >= b >= m and b * EPS <= CEILING for m, b in BOUNDS.values())
WORST = {}

S_CASES = rr.COMPOSITE_S            # (1, 63, 64, 65, 130, 192): one lane, a wave +- 1, ragged chunks
R_CASE, LIVE = rr.COMPOSITE_R, rr.COMPOSITE_LIVE   # 37 rays, 29 of them under a device-side count


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------- kernel cases
_CASES = {}


def _case(R, S, dev):
    """Inputs on the host and the device, the weights rsn_composite makes of them (what the forward reads) and the float64 references,
    computed once per shape and shared by the tests, which leave them unchanged."""
    key = (R, S)
    if key not in _CASES:
        inp = dr.distortion_inputs(R, S, dr.distortion_seed(S))
        d = {k: v.to(dev) for k, v in inp.items()}
        w = ops.composite(R, None, S, 0, 0, d["sigma"], d["eb"], torch.zeros(R, S, 3, device=dev), want_depth=False)["weights"]
        torch.cuda.synchronize()
        g_ref, g_scale, _ = dr.distortion_backward_reference(inp)
        ref = {"loss_ray": dr.loss_ray_reference(inp["sb"], w.cpu()), "g_sigma": g_ref, "g_scale": g_scale}
        if len(_CASES) > 6:
            _CASES.clear()
        _CASES[key] = (inp, d, w, ref)
    return _CASES[key]


def _forward(case, R, S, n_dev=None):
    _, d, w, _ = case
    out = _poisoned({"loss_ray": torch.empty(R, device=w.device)})["loss_ray"]
    check(_abi.load_library().rsn_distortion_forward(R, ptr(n_dev), S, ptr(d["sb"]), ptr(w), ptr(out), ops._stream()))
    torch.cuda.synchronize()
    return out


def _backward(case, R, S, accumulate, n_dev=None, into=None):
    _, d, w, _ = case
    out = _poisoned({"g_sigma": torch.empty(R, S, device=w.device)})["g_sigma"] if into is None else into
    check(_abi.load_library().rsn_distortion_backward(R, ptr(n_dev), S, ptr(d["sb"]), ptr(d["eb"]), ptr(d["sigma"]),
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
    bound = BOUNDS[name][1]
    print(f"RATIO {name} {ratio:.3f} [{label}] (bound {bound}, worst so far {WORST[name]:.3f})")
    assert ratio <= bound, f"{label} {name}: {ratio:.2f} x 2^-24 of the scale > {bound}"


def _is_poison(t):
    it, pattern = _POISON[t.dtype]
    return (t.view(it).reshape(t.shape[0], -1) == pattern).all(dim=1).cpu()


def _check_both(label, case, loss, g_sigma, rows=None):
    ref = case[3]
    _check(label, "loss_ray", loss, ref["loss_ray"], ref["loss_ray"] + rr.F32_TINY, rows=rows)
    _check(label, "g_sigma", g_sigma, ref["g_sigma"], ref["g_scale"], rows=rows)


@pytest.mark.parametrize("S", S_CASES)
def test_forward_and_backward_match_fp64(dev, S):
    """loss_ray against the O(S^2) double sum on the very weights the kernel read, g_sigma against fp64 autograd through w(sigma); every
    ray is compared, the planted ones included, and rays 0 and 1 are also held to their exact properties."""
    case = _case(R_CASE, S, dev)
    inp, _, w, _ = case
    loss, gs = _forward(case, R_CASE, S), _backward(case, R_CASE, S, 0)
    _check_both(f"S{S}", case, loss, gs)
    assert float(loss[0]) == 0.0 and bool((gs[0] == 0).all()), "the empty ray: loss and gradient are exactly 0"
    wc = w.cpu()
    assert float(wc[1, 0]) == 1.0 and bool((wc[1, 1:] == 0).all())  # saturated: all the weight in sample 0
    d0 = float(inp["sb"][1, 1].double() - inp["sb"][1, 0].double())
    assert abs(float(loss[1]) - d0 / 3) <= EPS * d0 / 3, "the saturated ray: L = w^2 d / 3, no inter-sample term"
    assert bool(torch.isfinite(gs[1]).all()) and bool((gs[1] == 0).all()), "the saturated ray: nothing behind an opaque sample"


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
    """29 of 37 rows: the rows under the count are written, the rows behind it are not touched.  accumulate = 0 starts from the poison
    pattern; accumulate = 1 from finite values (a NaN pattern would survive an addition), which must come back bit for bit."""
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


def test_repeatable_bits(dev):
    """No atomics and a fixed order of addition: two calls on the same inputs give the same bits."""
    S = 130
    case = _case(R_CASE, S, dev)
    assert torch.equal(_forward(case, R_CASE, S), _forward(case, R_CASE, S))
    assert torch.equal(_backward(case, R_CASE, S, 0), _backward(case, R_CASE, S, 0))


# ------------------------------------------------------------------------------------------------------------- the whole step
LAMBDA = 0.01  # weight of the distortion term in the oracle comparisons (mip-NeRF 360's); the test asserts that it matters at this size


def _dist_mean(sb, weights):
    """mean over the rays of the reference formula (the literal double sum, float64), differentiable in the oracle's weights [R,S,1]."""
    return dr.loss_ray_reference(sb, weights[..., 0]).mean()


def _oracle_weights(P, fs, rays, eb, detached, mean=None):
    """The oracle hands its weights out detached (cpu_ref.get_outputs).  This is its own computation of them once more -- field_level on
    the same bins (and contracted means), weights_from_density -- attached to the parameters, and equal to what it returned, bit for bit."""
    lv = cpu_ref.field_level(P, fs, *rays, eb, True, want_normals=False, mean_override=mean)
    w = cpu_ref.weights_from_density(lv["sigma"], lv["t0"], lv["t1"])
    assert torch.equal(w.detach(), detached)
    return w


def _density_head(grads):
    return torch.cat([grads["field_output_density.net.weight"].flatten(), grads["field_output_density.net.bias"].flatten()]).double()


@pytest.mark.parametrize("mma", ["f32", "bf16x6"])
def test_train_step_with_the_term_matches_oracle_autograd(dev, mma):
    """test_gpu_parity.test_train_forward_backward_matches_oracle_autograd on its smallest shape, with the distortion term on.
    (a) coarse level: the oracle's loss is that test's coarse loss + LAMBDA mean(reference formula on the oracle's own weights_coarse,
        re-attached by _oracle_weights, and its recorded coarse spacing bins), the HIP side's the same coarse loss + LAMBDA outputs.fused["dist_loss_ray_coarse"].mean(); the
        coarse samples are bit-identical, every parameter gradient within 2e-4 of the tensor's largest entry.  In the oracle the term
        must carry at least a tenth of the gradient norm of field_output_density, or this shows nothing.
    (b) both levels on identical positions (that test's part (c)): every parameter gradient within 5e-5."""
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
    model.config.loss_coefficients.update(distortion_loss_coarse=LAMBDA, distortion_loss_fine=LAMBDA)  # both levels on
    o, d, pa = cpu_ref.synthetic_rays(R, seed=seed + 50)
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    fs, ms = cpu_ref.FieldSpec(num_layers=layers, width=width), cpu_ref.ModelSpec(*samples)
    g = torch.Generator().manual_seed(seed + 1)
    jit = {"coarse": torch.rand(R, samples[0] + 1, generator=g), "fine": torch.rand(R, samples[1] + 1, generator=g),
           "reflect_coarse": torch.rand(R, samples[2] + 1, generator=g), "reflect_fine": torch.rand(R, samples[3] + 1, generator=g)}
    tgt = {k: torch.rand(R, 3, generator=g) for k in ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine")}
    tgt_dev = {k: v.to(dev) for k, v in tgt.items()}
    rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev), nears=nears.to(dev), fars=fars.to(dev))

    def oracle_grads():
        out = {k: p.grad.clone() for k, p in P.items() if p.grad is not None}
        for p in P.values():
            p.grad = None
        return out

    # ---- (a) coarse level
    rec = {}
    ref = cpu_ref.get_outputs(P, fs, ms, o, d, pa, nears, fars, training=True, jitter=jit, record_bins=rec)
    _coarse_loss(ref, tgt).backward(retain_graph=True)
    g_plain = oracle_grads()
    w_c = _oracle_weights(P, fs, (o, d, pa), rec["coarse_euclid"], ref["weights_coarse"])
    (_coarse_loss(ref, tgt) + LAMBDA * _dist_mean(rec["coarse_spacing"], w_c)).backward()
    g_ref = oracle_grads()
    share = float((_density_head(g_ref) - _density_head(g_plain)).norm() / _density_head(g_ref).norm())
    print(f"distortion term's share of the density head's gradient norm in the oracle: {share:.3f}")
    assert share >= 0.1, f"LAMBDA = {LAMBDA}: the distortion term is {share:.3f} of the density head's gradient; the comparison shows nothing"
    assert int(ref["mask"].sum()) > 0
    jit_gpu = dict(jit, reflect_coarse=jit["reflect_coarse"][ref["mask"]], reflect_fine=jit["reflect_fine"][ref["mask"]])
    model.zero_grad(set_to_none=True)
    out = model._get_outputs_train(rb, jitter=jit_gpu)
    assert set(out.fused) == set(train_graph.FUSED_KEYS) | set(train_graph.DIST_KEYS)
    checked = dict(out)
    checked["normals_coarse"] = ref["normals_coarse"].detach().to(dev)
    (_coarse_loss(checked, tgt_dev) + LAMBDA * out.fused["dist_loss_ray_coarse"].mean()).backward()
    torch.cuda.synchronize()
    want = dr.loss_ray_reference(rec["coarse_spacing"], ref["weights_coarse"][..., 0].detach())
    assert float((out.fused["dist_loss_ray_coarse"].detach().cpu().double() - want).abs().max()) <= 1e-5
    for name, p in model.field.named_parameters():
        gr = g_ref.get(name)
        if gr is None or float(gr.abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) <= 1e-12, name
            continue
        scale = float(gr.abs().max())
        err = float((p.grad.cpu() - gr).abs().max())
        assert err <= 2e-4 * scale + 1e-9, f"coarse loss + distortion, {name}: abs err {err:.3e}, scale {scale:.3e}"

    # ---- (b) both levels, the oracle evaluated at the kernels' own bins and contracted means
    model.zero_grad(set_to_none=True)
    model._keep_train_state = True
    out = model._get_outputs_train(rb, jitter=jit_gpu)
    st = model._train_state
    model._keep_train_state, model._train_state = False, None
    assert torch.equal(out["mask"].cpu(), ref["mask"])
    M = int(ref["mask"].sum())
    hip_bins, hip_means = {}, {}
    for name, sbk, ebk, lvk, n, S in (("coarse", "sb_c", "eb_c", "lc", R, samples[0]), ("fine", "sb_f", "eb_f", "lf", R, samples[1]),
                                      ("reflect_coarse", "sb_rc", "eb_rc", "lrc", M, samples[2]),
                                      ("reflect_fine", "sb_rf", "eb_rf", "lrf", M, samples[3])):
        hip_bins[name + "_spacing"], hip_bins[name + "_euclid"] = st[sbk].cpu(), st[ebk].cpu()
        hip_means[name] = st[lvk]["saved"]["enc"][:, 96:99].reshape(n, S, 3).cpu()
    ref2 = cpu_ref.get_outputs(P, fs, ms, o, d, pa, nears, fars, training=True, jitter=jit, bins=hip_bins, means=hip_means)
    w_c = _oracle_weights(P, fs, (o, d, pa), hip_bins["coarse_euclid"], ref2["weights_coarse"], hip_means["coarse"])
    w_f = _oracle_weights(P, fs, (o, d, pa), hip_bins["fine_euclid"], ref2["weights_fine"], hip_means["fine"])
    (_loss_from_outputs(ref2, tgt) + LAMBDA * (_dist_mean(hip_bins["coarse_spacing"], w_c)
                                               + _dist_mean(hip_bins["fine_spacing"], w_f))).backward()
    g_ref = oracle_grads()
    checked = dict(out)
    checked["normals_coarse"] = ref2["normals_coarse"].detach().to(dev)
    checked["normals_fine"] = ref2["normals_fine"].detach().to(dev)
    (_loss_from_outputs(checked, tgt_dev) + LAMBDA * (out.fused["dist_loss_ray_coarse"].mean()
                                                      + out.fused["dist_loss_ray_fine"].mean())).backward()
    torch.cuda.synchronize()
    worst = (0.0, "")
    for name, p in model.field.named_parameters():
        if "field_output_low" in name:
            assert p.grad is None and name not in g_ref
            continue
        gr = g_ref[name]
        worst = max(worst, (float((p.grad.cpu() - gr).abs().max()) / float(gr.abs().max()), name))
    print(f"identical positions, full loss + both distortion terms ({mma}): worst gradient error / tensor max {worst[0]:.2e} ({worst[1]})")
    assert worst[0] <= 5e-5, f"identical positions: {worst[1]} off by {worst[0]:.3e} of its largest entry"


def test_bf16_step_with_the_term(dev):
    """The reduced-precision mode consumes the same fp32 g_sigma: one step with the term on yields finite gradients, and what the term
    adds to the density head's gradient (on minus off, same injected jitter) points where the exact-fp32 run's addition points."""
    R = 96
    g = torch.Generator().manual_seed(3)
    jit = {"coarse": torch.rand(R, 17, generator=g), "fine": torch.rand(R, 17, generator=g),
           "reflect_coarse": torch.rand(R, 9, generator=g), "reflect_fine": torch.rand(R, 9, generator=g)}
    image = torch.rand(R, 3, generator=g).to(dev)
    delta = {}
    for mode in ("f32", "bf16"):
        grads = {}
        for on in (False, True):
            torch.manual_seed(11)
            cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=16, num_importance_samples=16,
                                                    num_reflect_coarse_samples=8, num_reflect_importance_samples=8)
            model = cfg.setup(scene_box=None, num_train_data=1)
            with torch.no_grad():
                model.field.field_output_density.net.bias += 2.0
            model.to(dev).train()
            model.field.set_mma_mode(mode)
            if on:
                model.config.loss_coefficients.update(distortion_loss_coarse=1.0, distortion_loss_fine=1.0)
            o, d, pa = cpu_ref.synthetic_rays(R, seed=21)
            rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev),
                               nears=torch.full((R, 1), 2.0, device=dev), fars=torch.full((R, 1), 6.0, device=dev))
            out = model._get_outputs_train(rb, jitter=jit)
            sum(model.get_loss_dict(out, {"image": image}).values()).backward()
            torch.cuda.synchronize()
            grads[on] = {n: p.grad.detach().cpu().clone() for n, p in model.field.named_parameters() if p.grad is not None}
            assert all(bool(torch.isfinite(v).all()) for v in grads[on].values()), (mode, on)
        delta[mode] = _density_head(grads[True]) - _density_head(grads[False])
        assert float(delta[mode].norm()) > 0.1 * float(_density_head(grads[True]).norm()), "the term does not reach the density head"
    cos = float(torch.dot(delta["bf16"], delta["f32"]) / (delta["bf16"].norm() * delta["f32"].norm()))
    print(f"bf16 vs f32, the term's addition to the density head's gradient: cosine {cos:.5f}")
    assert cos >= 0.99


# ------------------------------------------------------------------------------------------------------------- loss dictionary
def test_loss_dict_keys_and_the_off_path_bits(dev):
    """Absent and 0.0 coefficients: exactly the eight reference keys, outputs.fused holds FUSED_KEYS only, and under the deterministic
    mode the parameter gradients of the two are the same bits.  Both set: ten keys, device tensors, coef * mean."""
    model, rb, batch = _train_setup(dev, 64, (16, 16, 8, 8), layers=4, width=64)
    model.set_deterministic(True)
    coef = model.config.loss_coefficients
    grads = []
    for zeros in (False, True):
        coef.pop("distortion_loss_coarse", None), coef.pop("distortion_loss_fine", None)
        if zeros:
            coef.update(distortion_loss_coarse=0.0, distortion_loss_fine=0.0)
        model.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        out = model(rb)
        assert set(out.fused) == set(train_graph.FUSED_KEYS)
        ld = model.get_loss_dict(out, batch)
        assert tuple(ld) == train_ops.LOSS_TERMS
        sum(ld.values()).backward()
        grads.append({n: p.grad.clone() for n, p in model.field.named_parameters() if p.grad is not None})
    assert sorted(grads[0]) == sorted(grads[1]) and all(torch.equal(grads[0][n], grads[1][n]) for n in grads[0])
    coef.update(distortion_loss_coarse=0.5, distortion_loss_fine=0.25)
    torch.manual_seed(5)
    out = model(rb)
    assert tuple(out.fused) == train_graph.FUSED_KEYS + train_graph.DIST_KEYS
    ld = model.get_loss_dict(out, batch)
    assert tuple(ld) == train_ops.LOSS_TERMS + ("distortion_loss_coarse", "distortion_loss_fine") and len(ld) == 10
    for key, ray_key, c in (("distortion_loss_coarse", "dist_loss_ray_coarse", 0.5), ("distortion_loss_fine", "dist_loss_ray_fine", 0.25)):
        assert ld[key].is_cuda and ld[key].dim() == 0 and ld[key].requires_grad
        want = c * float(out.fused[ray_key].detach().double().mean())
        assert abs(float(ld[key].detach()) - want) <= 1e-6 * want and want > 0


# ------------------------------------------------------------------------------------------------------------- train_step
def test_chunked_train_step_equals_whole_batch_step_with_the_term(dev):
    """test_gpu_parity.test_chunked_train_step_equals_whole_batch_step with both distortion terms on, at its bounds: the terms are
    means over the rays (parallel._MEAN_TERMS), a chunk of m of R rays enters with weight m / R."""
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
            model.config.loss_coefficients.update(distortion_loss_coarse=0.5, distortion_loss_fine=1.0)
            o, d, pa = cpu_ref.synthetic_rays(R, seed=3)
            rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev),
                               nears=torch.full((R, 1), 2.0, device=dev), fars=torch.full((R, 1), 6.0, device=dev))
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
    """The method of test_gpu_parity.test_training_step_issues_no_device_to_host_read, with both distortion terms on."""
    from reflect_sampling_nerf_amd.parallel import train_step

    model, rb, batch = _train_setup(dev, 192, (24, 24, 16, 16))
    model.config.loss_coefficients.update(distortion_loss_coarse=0.002, distortion_loss_fine=0.01)
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


@pytest.fixture(scope="module")
def scene():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return _sphere_scene(6)


@pytest.fixture(scope="module")
def run_six(scene, tmp_path_factory):
    """6 deterministic steps with --distortion-loss X (checkpoints at steps 3 and 5): trained once, read by both trainer tests."""
    return _Run(scene, tmp_path_factory.mktemp("dist_a"), steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True,
                distortion_loss=X)


def test_trainer_runs_are_bit_reproducible_with_the_term(scene, run_six, tmp_path):
    """Two deterministic runs of 6 steps with the term: identical parameters and moments.  The run records the coefficient, its first
    log line names it, and it differs from the run without the term (which records nothing)."""
    again = _Run(scene, tmp_path / "b", steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True, distortion_loss=X)
    assert _differing(run_six.ckpt(5), again.ckpt(5)) == []
    rs = _load(run_six.ckpt(5))["rsn_run"]
    assert rs["distortion_loss"] == X and "distortion_loss_coarse" not in rs and rs["version"] == 1
    assert "distortion_loss_fine 0.01" in run_six.logs[0] and "distortion_loss_coarse" not in run_six.logs[0]
    plain = _Run(scene, tmp_path / "c", steps=6, save_every=3, rays=96, mma="f32", seed=0, deterministic=True)
    assert "distortion" not in plain.logs[0] and not any(k.startswith("distortion") for k in _load(plain.ckpt(5))["rsn_run"])
    assert any(k.startswith("pipeline/") for k in _differing(run_six.ckpt(5), plain.ckpt(5))), "the term changed nothing"


def test_trainer_resume_restores_the_coefficient_bit_exactly(scene, run_six, tmp_path):
    """3 steps, then --resume to 6 WITHOUT the flag: the coefficient comes from the checkpoint and the result is the uninterrupted run's."""
    first = _Run(scene, tmp_path / "d", steps=3, save_every=0, rays=96, mma="f32", seed=0, deterministic=True, distortion_loss=X)
    assert first.saved_steps() == [2]
    rest = _Run(scene, tmp_path / "d", steps=6, save_every=3, resume=first.ckpt(2))
    assert "distortion_loss_fine 0.01" in rest.logs[0]
    assert _differing(run_six.ckpt(5), rest.ckpt(5)) == []
    assert all(torch.equal(run_six.losses[s], rest.losses[s]) for s in (3, 4, 5))
    assert _load(rest.ckpt(5))["rsn_run"]["distortion_loss"] == X
