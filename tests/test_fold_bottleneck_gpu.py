"""The exact-fp32 training kernels with field_output_bottleneck folded into mlp_mid (RSN_MMA_F32_FOLDED), on the GPU.

field_output_bottleneck is a Linear with no activation whose only consumer is the x part of mlp_mid.layers.0, so the folded kernels
run ONE affine map W_c = W_mx W_b, b_c = b_mid + W_mx b_b (formed in fp64 when the weights are packed) where the two-GEMM kernels
run two.  Checked here: the gradient-recovery kernel alone against an fp64 product; every row the folded forward / backward write
against the two-GEMM kernels on the same inputs (the trunk, the heads and everything upstream of the colour path bit for bit, the
colour path within the suite's fp32-equivalence bound); the persistent loop and a three-job launch against the fp64 oracle; and the
parameter gradients of a whole small step, folded against two-GEMM, plus their bits from run to run in the ordered mode."""
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, ops, train_graph
from reflect_sampling_nerf_amd._abi import check, ptr
from tests.helpers import check_points, multitile_geometry, point_err

pytestmark = pytest.mark.gpu

EQUIV = 2e-6  # the suite's fp32-equivalence bound, / the tensor's largest value (test_gpu_parity: split-bf16 rows vs exact rows)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


# ---------------------------------------------------------------------------------------------- 1. the unfold kernel alone
@pytest.mark.parametrize("w,ld_c", [(256, 256), (200, 256), (64, 64)])
def test_unfold_kernel_against_fp64(dev, w, ld_c):
    """rsn_unfold_bottleneck_grads on random C, s and weights (200: the parameters of a param_width = 200 field, C rows 256 apart)
    ADDS dW_b = W_mx^T C, db_b = W_mx^T s and dW_mx = C W_b^T + s (x) b_b to what the gradient tensors hold.  Bound: 2^-22 of each
    output's largest entry -- the kernel rounds an fp64 sum to fp32 once (2^-24 of the sum) and adds it in fp32 (2^-24 of the
    result); the columns of d_mid_w outside [34, 34 + w) keep their bits."""
    lib = _abi.load_library()
    g = torch.Generator().manual_seed(w)
    ld_mid = 34 + w
    cbuf = torch.randn(128, ld_c, generator=g)
    s = torch.randn(128, generator=g)
    mid_w = torch.randn(128, ld_mid, generator=g) / 16.0
    bott_w, bott_b = torch.randn(w, w, generator=g) / 16.0, torch.randn(w, generator=g)
    init = {"bw": torch.randn(w, w, generator=g), "bb": torch.randn(w, generator=g), "mw": torch.randn(128, ld_mid, generator=g)}
    out = {k: v.clone().to(dev) for k, v in init.items()}
    dv = lambda t: t.to(dev)  # noqa: E731
    c_d, s_d, mw_d, bw_d, bb_d = dv(cbuf), dv(s), dv(mid_w), dv(bott_w), dv(bott_b)
    check(lib.rsn_unfold_bottleneck_grads(w, 128, ptr(c_d), ld_c, ptr(s_d), ptr(mw_d), ld_mid, ptr(bw_d), ptr(bb_d),
                                          ptr(out["bw"]), ptr(out["bb"]), ptr(out["mw"]), ops._stream()))
    torch.cuda.synchronize()
    c64, s64, wmx = cbuf[:, :w].double(), s.double(), mid_w[:, 34:].double()
    ref = {"bw": init["bw"].double() + wmx.t() @ c64, "bb": init["bb"].double() + wmx.t() @ s64, "mw": init["mw"].double()}
    ref["mw"][:, 34:] += c64 @ bott_w.double().t() + s64[:, None] * bott_b.double()[None, :]
    assert torch.equal(out["mw"][:, :34].cpu(), init["mw"][:, :34])
    for k in ref:
        err, top = float((out[k].double().cpu() - ref[k]).abs().max()), float(ref[k].abs().max())
        print(f"unfold w={w} {k}: err {err:.3e}, largest entry {top:.3e}, ratio {err / top:.3e} (bound {2.0 ** -22:.3e})")
        assert err <= 2.0 ** -22 * top, k
    # the same inputs give the same bits
    again = {k: v.clone().to(dev) for k, v in init.items()}
    check(lib.rsn_unfold_bottleneck_grads(w, 128, ptr(c_d), ld_c, ptr(s_d), ptr(mw_d), ld_mid, ptr(bw_d), ptr(bb_d),
                                          ptr(again["bw"]), ptr(again["bb"]), ptr(again["mw"]), ops._stream()))
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], again[k]) for k in out)


# ---------------------------------------------------------------------------------------------- 2. rows, folded vs two-GEMM
def _rows_case(dev, width, R=37, S=32):
    torch.manual_seed(0)
    f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=8, base_mlp_layer_width=width)
    with torch.no_grad():
        f.field_output_density.net.bias += 2.0
    f = f.to(dev).train()
    o, d, pa = cpu_ref.synthetic_rays(R, seed=1)
    o, d, pa = o.to(dev), d.to(dev), pa.to(dev).reshape(-1)
    bins = (2.0 + 4.0 * torch.linspace(0, 1, S + 1)).repeat(R, 1).to(dev).contiguous()
    gen = torch.Generator().manual_seed(3)
    gin = {"sigma": torch.randn(R, S, generator=gen).to(dev), "color": torch.randn(R, S, 3, generator=gen).to(dev),
           "pred_normals": torch.randn(R, S, 3, generator=gen).to(dev), "n_dot_d": torch.randn(R, S, generator=gen).to(dev),
           "roughness": torch.randn(R, S, generator=gen).to(dev)}
    return f, (o, d, pa), bins, gin


@pytest.mark.parametrize("want_normals,need_input", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("width", [256, 64, 200])
def test_folded_rows_match_the_two_gemm_kernels(dev, width, want_normals, need_input):
    """37 x 32 = 1,184 points (nine full 128-point tiles and one with two live waves; the shape of
    test_split_bf16_ring_rows_match_the_exact_kernels_and_repeat_bitwise) at widths 256, 64 and param_width 200 inside 256.
    Bit for bit: every output and saved row upstream of the colour path (the raw heads of saved.heads are its first four columns;
    the other live ones hold the mid RGB, which is colour path) and the trunk's ReLU bits.  Within 2e-6 of the tensor's largest value:
    colour, saved.hid, the mid RGB and every gradient row.  A point whose mlp_mid ReLU bits differ between the two forms (a
    pre-activation within reassociation of zero) is left out of the gradient rows; at most 2 of the 1,184 may be."""
    f, rays, bins, gin = _rows_case(dev, width)
    L, N = 8, bins.shape[0] * (bins.shape[1] - 1)
    res = {}
    for fold in (False, True):
        lv = f.evaluate_frustums_train(*rays, bins, want_normals=want_normals, fold=fold)
        go = train_graph._field_backward(f, rays, bins, lv, gin, need_input, fold=fold)
        torch.cuda.synchronize()
        res[fold] = (lv, go)
    (la, ga), (lb, gb) = res[False], res[True]
    assert "bott" in la["saved"] and "bott" not in lb["saved"] and "d_bott" in ga and "d_bott" not in gb
    for k in ("sigma", "raw_density", "pred_normals", "n_dot_d", "diff", "tint", "roughness") + (("normals",) if want_normals else ()):
        assert torch.equal(la[k], lb[k]), k
    assert torch.equal(la["saved"]["act"], lb["saved"]["act"]) and torch.equal(la["saved"]["enc"], lb["saved"]["enc"])
    assert torch.equal(la["saved"]["sh"], lb["saved"]["sh"])
    assert torch.equal(la["saved"]["heads"][:, :4], lb["saved"]["heads"][:, :4])
    nw = f.width // 64  # mask words a lane half writes per trunk layer (the buffer holds at least 2; mlp_mid's four blocks: 2)
    assert torch.equal(la["saved"]["relu_bits"][:L, :, :, :nw], lb["saved"]["relu_bits"][:L, :, :, :nw])

    def close(name, a, b, keep=None):
        a, b = a.double(), b.double()
        if keep is not None:
            a, b = a[..., keep, :], b[..., keep, :]
        err, top = float((a - b).abs().max()), max(float(a.abs().max()), 1e-3)
        print(f"fold rows W={width} {name}: {err / top:.3e} of the largest value (bound {EQUIV:.0e})")
        assert err <= EQUIV * top, name

    close("color", la["color"].reshape(N, 3), lb["color"].reshape(N, 3))
    close("saved.hid", la["saved"]["hid"], lb["saved"]["hid"])
    close("saved.heads[:, 4:7] (mid RGB)", la["saved"]["heads"][:, 4:7], lb["saved"]["heads"][:, 4:7])
    flip = (la["saved"]["relu_bits"][L, :, :, :2] != lb["saved"]["relu_bits"][L, :, :, :2]).reshape(N, -1).any(dim=1)
    print(f"fold rows W={width}: {int(flip.sum())} of {N} points with an mlp_mid ReLU unit on the other side of zero")
    assert int(flip.sum()) <= 2
    keep = ~flip
    for k in ("da_mid", "dz_rgb", "dz_heads") + (("d_input",) if need_input else ()):
        close("gout." + k, ga[k].reshape(N, -1), gb[k].reshape(N, -1), keep)
    for l in range(L):
        close(f"gout.dy[{l}]", ga["dy"][l], gb["dy"][l], keep)


# ---------------------------------------------------------------------------------------------- 3. the persistent loop vs fp64
class _Folded:
    """A Field as the folded kernels see it: descriptor, packed weights and saved buffers of fold=True, everything else its own."""

    def __init__(self, f):
        self._f = f

    def __getattr__(self, name):
        return getattr(self._f, name)

    def field_desc(self):
        return self._f.field_desc(True)

    def packed_weights(self):
        return self._f.packed_weights(True)

    def alloc_saved(self, n, dev):
        return self._f.alloc_saved_folded(n, dev)


def _fold_grads(f, evals):
    acc = train_graph._GradAcc(f)
    train_graph._weight_grads(f, evals, acc, fold=True)
    return {k: v.clone() for k, v in acc.finish().items()}


def test_folded_level_multitile_against_fp64(dev, cus):
    """One f32 8 x 256 training level on the folded kernels at test_multitile_gpu's size (787 x 250 points: every workgroup walks
    >= 3 tiles, ragged last tile, tile count no multiple of the grid) against that module's fp64 oracle run (shared, computed
    once per session) with its bounds.  What is shared is the oracle's host-side result: the exact-fp32 GPU rows that building the
    case leaves in that module's cache (4 GB of saved and gradient rows) are dropped again here -- this file runs ahead of
    test_gpu_parity, whose memory test reads the process's allocated bytes; test_multitile_gpu re-runs its launch when it gets there."""
    import test_multitile_gpu as mt  # pytest's own module object (rootdir-less tests directory): one oracle cache

    built_here = 256 not in mt._level_cache
    case = mt._level_case(dev, 256)
    if built_here:
        case["gpu"].pop("f32", None)
    R, S, f = case["R"], case["S"], case["f"]
    N, tile, label = R * S, 128, "folded level f32 8x256"
    _, grid, _ = multitile_geometry(label, [N], tile, cus)
    f.set_mma_mode("f32")
    o, d, pa = case["rays"]
    lv = f.evaluate_frustums_train(o, d, pa, case["eb"], want_normals=True, fold=True)
    go = train_graph._field_backward(f, (o, d, pa), case["eb"], lv, case["gin"], True, fold=True)
    grads = _fold_grads(f, [(lv["saved"], go, True)])
    torch.cuda.synchronize()
    assert torch.equal(mt.saved_means(f, lv["saved"]).cpu(), case["means"])
    ref = case["ref"]
    for k in ("sigma", "color", "pred_normals", "n_dot_d", "diff", "tint", "roughness"):
        check_points(label, k, point_err(lv[k], ref[k], N), mt.TOL_UNIT if k in ("pred_normals", "n_dot_d") else mt.TOL, tile, grid)
    mt.check_normals(label, point_err(lv["normals"], ref["normals"], N), tile, grid)
    scale = float(case["dpa"].abs().max())
    check_points(label, "d_input / max|d_input|", point_err(go["d_input"], case["dpa"], N) / scale, mt.D_INPUT_F32, tile, grid)
    mt.check_param_grads(label, f, grads, case["gref"])


def test_folded_three_job_launch_against_fp64(dev, cus):
    """rsn_field_forward_train_jobs / rsn_field_backward_jobs on the folded kernels with the reflect branch's shape (two frustum
    levels and get_inf_color; the sizes of test_multitile_gpu.test_jobs_launches_equal_separate_launches: job boundaries inside a
    later round and off tile boundaries): every job's outputs, input gradient and parameter gradients against the fp64 oracle."""
    import test_multitile_gpu as mt  # pytest's own module object (rootdir-less tests directory): one oracle cache

    f, P, fs = mt._field(dev, 256, seed=21)
    f.set_mma_mode("f32")
    jobs, host = [], []
    for R, S, seed in ((301, 130, 31), (263, 190, 32)):
        o, d, pa, eb = mt._rays(R, S, seed)
        gin = mt._gin(R * S, seed + 1)
        host.append((o, d, pa, eb, gin))
        jobs.append({"kind": 0, "rays": (o.to(dev), d.to(dev), pa.reshape(R).to(dev), eb.to(dev)),
                     "gin": {kk: v.reshape((R, S) + v.shape[1:]).to(dev) for kk, v in gin.items()}, "n": R * S})
    dirs, sq, g_rgb = mt._inf_inputs(14000, 33, dev)
    jobs.append({"kind": 1, "inf": (dirs.to(dev), sq.to(dev)), "g_rgb": g_rgb.to(dev), "n": dirs.shape[0]})
    tile, label = 128, "folded jobs f32"
    _, grid, base = multitile_geometry(label, [j["n"] for j in jobs], tile, cus)
    ff = _Folded(f)
    fwd = mt._fwd_jobs(ff, jobs, dev)
    bwd = mt._bwd_jobs(ff, jobs, fwd, dev)
    torch.cuda.synchronize()
    for q, (job, lv, go) in enumerate(zip(jobs, fwd, bwd)):
        n, lab = job["n"], f"{label} job {q}"
        grads = _fold_grads(f, [(lv["saved"], go, job["kind"] == 0)])
        if job["kind"] == 0:
            o, d, pa, eb, gin = host[q]
            ref, gref, dpa = mt.oracle_points(P, fs, o, d, pa, eb, gin, mt.saved_means(f, lv["saved"]).cpu())
            for k in ("sigma", "color", "pred_normals", "n_dot_d", "diff", "tint", "roughness"):
                check_points(lab, k, point_err(lv[k], ref[k], n), mt.TOL_UNIT if k in ("pred_normals", "n_dot_d") else mt.TOL,
                             tile, grid, base[q])
        else:
            rgb, gref, dpa = mt.oracle_inf(P, fs, dirs, sq, g_rgb)
            check_points(lab, "rgb", point_err(lv["rgb"], rgb, n), mt.INF_F32, tile, grid, base[q])
        check_points(lab, "d_input / max", point_err(go["d_input"], dpa, n) / float(dpa.abs().max()), mt.D_INPUT_F32, tile, grid,
                     base[q])
        mt.check_param_grads(lab, f, grads, gref)


# ---------------------------------------------------------------------------------------------- 4. a whole small step
def _small_step(dev, fold, ordered):
    """One training step (forward, the eight-term loss, backward) of a fresh 8 x 256 model on 192 rays x (24 + 24) + reflect 16 + 16
    (test_gpu_parity._train_setup's small size), same seeds and draws every time -> (loss, parameter gradients)."""
    torch.manual_seed(0)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=24, num_importance_samples=24, num_reflect_coarse_samples=16,
                                            num_reflect_importance_samples=16, base_mlp_num_layers=8, base_mlp_layer_width=256)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 2.0
    model.to(dev).train()
    model.set_deterministic(ordered)
    model.fold_bottleneck = fold
    R = 192
    o, d, pa = cpu_ref.synthetic_rays(R, seed=0)
    rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev),
                       nears=torch.full((R, 1), 2.0, device=dev), fars=torch.full((R, 1), 6.0, device=dev))
    batch = {"image": torch.rand(R, 3, generator=torch.Generator().manual_seed(1)).to(dev)}
    torch.manual_seed(7)
    out = model(rb)
    assert 0 < int(out["mask"].sum()) < R
    loss = sum(model.get_loss_dict(out, batch).values())
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: p.grad.clone() for n, p in model.field.named_parameters() if p.grad is not None}


def test_small_step_folded_against_two_gemm_and_repeatable(dev):
    """Fold on against fold off on the same seeds and jitter: the loss within 1e-6 relative, every parameter gradient within 2e-5
    of its tensor's largest entry (the weight-gradient bound of test_weight_grad_mma_modes).  With the ordered weight-gradient mode
    two folded runs give the same bits in every gradient."""
    l_off, g_off = _small_step(dev, False, False)
    l_on, g_on = _small_step(dev, True, False)
    print(f"small step: loss two-GEMM {l_off:.9g}, folded {l_on:.9g}, relative difference {abs(l_on - l_off) / abs(l_off):.3e}")
    assert abs(l_on - l_off) <= 1e-6 * abs(l_off)
    assert sorted(g_on) == sorted(g_off)
    worst = (0.0, "")
    for n in g_off:
        worst = max(worst, (float((g_on[n] - g_off[n]).abs().max()) / (float(g_off[n].abs().max()) + 1e-30), n))
    print(f"small step: worst parameter-gradient difference {worst[0]:.3e} of the tensor's largest entry ({worst[1]}; bound 2e-5)")
    assert worst[0] <= 2e-5, worst
    l_a, g_a = _small_step(dev, True, True)
    l_b, g_b = _small_step(dev, True, True)
    assert l_a == l_b
    for n in g_a:
        assert torch.equal(g_a[n], g_b[n]), f"ordered mode: gradient of {n} differs between two folded runs"
