"""The persistent field kernels where a workgroup walks several tiles, against the oracle in float64.

Every field kernel is persistent: grid = min(tiles, CUs) and each workgroup loops `gtile += gridDim.x`.  What only the
second and later iterations do -- the LDS weight ring's walk position and counters carried across tiles, bias tables written
once per workgroup, the job of a tile looked up through the tile boundaries of a multi-job launch -- is checked here at sizes
where every workgroup runs at least three iterations, the last tile is ragged and the tile count is not a multiple of the
grid (tests/helpers.multitile_geometry asserts that for each launch).  The reference is oracle/cpu_ref.py evaluated in float64
(parameters and inputs cast); gradients come from float64 autograd through it.  A failing comparison names the worst point,
its tile and its persistent-loop iteration (tile // grid)."""
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, ops, train_graph
from reflect_sampling_nerf_amd._abi import FieldGradsIn, check, ptr
from tests.helpers import _POISON, _poisoned, check_points, default_dtype, locate, multitile_geometry, point_err, tile_rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4       # test_gpu_parity.TOL: continuous outputs
TOL_UNIT = 5e-4  # test_gpu_parity.TOL_UNIT: predicted normals and n.d
TOL_BF16 = 3e-2  # the plain-bf16 modes' tolerance (test_gpu_parity: bf16 sweeps, configs[3])
TILE = {"f32": 128, "bf16x6": 128, "bf16": 256}  # points per tile of the training kernels at width 256, per MMA mode
# Bounds measured on MI355X (worst case over the cases of this file), set at about 4x the measurement.  Gradients against
# fp64 at these sizes: the kernels' fp32 pre-activations differ from fp64 by ~1e-6, so over ~1e8 hidden units a few hundred
# ReLU units near zero switch side, each moving its point's gradient by O(1); the per-point input gradient and the parameter
# gradients (sums over 1e5 points with random upstream signs) carry that.  Forward values have no such discontinuity.
D_INPUT_F32 = 3e-1     # d_input / d_sqradius vs fp64, / largest entry (f32, bf16x6): measured 7.9e-2
D_INPUT_BF16 = 5e-1    # the same in plain bf16: measured 1.2e-1
GRAD_F32 = 7e-2        # parameter gradients vs fp64, / tensor max, one level or get_inf_color (f32, bf16x6): measured 1.7e-2
ROWS_BF16 = 5.5e-1     # plain-bf16 rows vs the exact kernels, relative L2 per 256-point tile: measured 1.4e-1 (d_input; dy 1.3e-1)
GRAD_BF16_COS = 3e-2   # plain-bf16 parameter gradients vs fp64: 1 - cosine, measured 7.3e-3
GRAD_BF16_REL = 5e-1   # ... relative L2, measured 1.2e-1
ROWS_X6 = 8e-6         # split-bf16 rows vs the exact kernels, / tensor max: measured 2.07e-6 (2.0e-6 within iteration 0;
                       # test_gpu_parity's 2e-6 bound holds at 1,184 points, the tail of 196,750 points reaches just past it)
GRAD_STEP = 2e-2      # parameter gradients vs fp64, / tensor max, whole steps on the ray subset: measured 4.7e-3
# analytic normals vs fp64 (unit vectors through a division by a raw-density gradient that can be tiny; test_gpu_parity's
# 1e-3 / 5e-3 rule is against the fp32 oracle, which shares the kernels' fp32 rounding of the IPE arguments):
# mean |error| and its 0.99-quantile, measured 8.3e-3 / 1.6e-1 (f32, bf16x6; worst: a whole step's fine level), 3.4e-2 (bf16)
NORMALS_MEAN, NORMALS_Q99 = 3.5e-2, 6.5e-1
NORMALS_BF16 = 1.5e-1                  # plain bf16: mean |error|
INF_F32 = 5e-6         # get_inf_color colour vs fp64 (f32, bf16x6): measured 1.1e-6
CFG3_FP64 = 2.5e-4     # configs[3] bf16 eval colour vs fp64: measured 5.9e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _field(dev, width, seed, bias_shift=1.0):
    torch.manual_seed(seed)
    f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=8, base_mlp_layer_width=width)
    with torch.no_grad():
        f.field_output_density.net.bias += bias_shift
    P = {k: v.detach().clone() for k, v in f.state_dict().items()}
    return f.to(dev).train(), P, cpu_ref.FieldSpec(num_layers=8, width=width)


def _rays(R, S, seed):
    """Rays, per-ray pixel areas spread over two decades (the input gradient flows through the IPE variance) and jittered
    uniform bins on [2, 6].  (Far smaller areas leave IPE frequencies up to 2^16 undamped, whose fp32 phase is off by
    ~1e-2 rad: that is fp32's limit, not a kernel's, and it would swamp the per-point input gradient.)"""
    g = torch.Generator().manual_seed(seed)
    o, d, _ = cpu_ref.synthetic_rays(R, seed=seed)
    pa = 10.0 ** (-4.0 + 2.0 * torch.rand(R, 1, generator=g))
    _, eb = cpu_ref.spaced_bins("uniform", 1.0, torch.full((R, 1), 2.0), torch.full((R, 1), 6.0), S,
                                torch.rand(R, S + 1, generator=g))
    return o, d, pa, eb.contiguous()


def _gin(N, seed):
    g = torch.Generator().manual_seed(seed)
    return {"sigma": torch.randn(N, generator=g), "color": torch.randn(N, 3, generator=g),
            "pred_normals": torch.randn(N, 3, generator=g), "n_dot_d": torch.randn(N, generator=g),
            "roughness": torch.randn(N, generator=g)}


def _param_grads_fp64(P64):
    return {k: (None if p.grad is None else p.grad.detach()) for k, p in P64.items()}


def oracle_points(P, fs, o, d, pa, eb, gin, means, chunk=16384):
    """fp64 cpu_ref.field_level on every point of [R, S] samples, in training mode with analytic normals, at the contracted
    means [N, 3] the kernels used (as test_gpu_parity's test_train_forward_backward_matches_oracle_autograd (c): an ulp of the
    fp32 mean moves the undamped IPE frequencies by ~1e-4; the covariance, which carries the pixel-area gradient, is computed
    here).  Each point is evaluated as a one-sample ray (the field is pointwise), so d loss / d pixel_area comes out per point,
    as the kernels' d_input.  Loss = sum(gin . (sigma, color, pred_normals, n_dot_d, sigmoid(roughness head))).
    -> (per-point outputs, parameter gradients, d loss / d pixel_area [N])."""
    R, S = eb.shape[0], eb.shape[1] - 1
    N = R * S
    with default_dtype(torch.float64):
        P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
        op, dp = o.double().repeat_interleave(S, 0), d.double().repeat_interleave(S, 0)
        pap = pa.double().reshape(R).repeat_interleave(S)
        ebp = torch.stack([eb[:, :-1].reshape(N), eb[:, 1:].reshape(N)], 1).double()
        outs, d_pa = {}, []
        for lo in range(0, N, chunk):
            sl = slice(lo, min(N, lo + chunk))
            n = sl.stop - lo
            pa_c = pap[sl].reshape(n, 1).clone().requires_grad_(True)
            lv = cpu_ref.field_level(P64, fs, op[sl], dp[sl], pa_c, ebp[sl], training=True, want_normals=True,
                                     mean_override=means[sl].double().reshape(n, 1, 3))
            y = {"sigma": lv["sigma"], "color": lv["color"], "pred_normals": lv["pred_normals"], "n_dot_d": lv["n_dot_d"],
                 "roughness": torch.sigmoid(lv["rough_raw"])}
            sum((gin[k][sl].double().reshape(n, -1) * v.reshape(n, -1)).sum() for k, v in y.items()).backward()
            d_pa.append(pa_c.grad.reshape(n))
            y.update(diff=lv["diff"], tint=lv["tint"], normals=lv["normals"])
            for k, v in y.items():
                outs.setdefault(k, []).append(v.detach().reshape(n, -1))
        outs = {k: torch.cat(v) for k, v in outs.items()}
        return outs, _param_grads_fp64(P64), torch.cat(d_pa)


def oracle_inf(P, fs, dirs, sq, g_rgb, chunk=32768):
    """fp64 cpu_ref.inf_color and the gradients of sum(g_rgb . rgb): -> (rgb, parameter gradients, d / d sqradius [M])."""
    M = dirs.shape[0]
    with default_dtype(torch.float64):
        P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
        rgb, dsq = [], []
        for lo in range(0, M, chunk):
            sl = slice(lo, min(M, lo + chunk))
            sq64 = sq[sl].double().reshape(-1, 1).clone().requires_grad_(True)
            c = cpu_ref.inf_color(P64, fs, dirs[sl].double(), sq64)
            (g_rgb[sl].double() * c).sum().backward()
            rgb.append(c.detach())
            dsq.append(sq64.grad.reshape(-1))
        return torch.cat(rgb), _param_grads_fp64(P64), torch.cat(dsq)


def check_normals(label, e, tile, grid, bf16=False):
    """Analytic normals: mean and 0.99-quantile of the per-point errors, and where the worst one sits."""
    e_mean, e_q = float(e.mean()), float(e.quantile(0.99))
    w, i, t, it, e0, e1 = locate(e, tile, grid)
    print(f"[{label}] normals: mean {e_mean:.3e}, 0.99-quantile {e_q:.3e}; worst {w:.3e} at point {i}, tile {t}, iteration {it}")
    if bf16:
        assert e_mean <= NORMALS_BF16, f"{label}: analytic normals mean error {e_mean:.3e}"
    else:
        assert e_mean <= NORMALS_MEAN and e_q <= NORMALS_Q99, \
            f"{label}: analytic normals mean {e_mean:.3e}, 0.99-quantile {e_q:.3e} (worst at tile {t}, iteration {it})"


def weight_grads(f, evals):
    """The production weight-gradient path (train_graph._weight_grads) over [(saved, gout, with_heads)]."""
    acc = train_graph._GradAcc(f)
    train_graph._weight_grads(f, evals, acc)
    return acc.finish()


def check_param_grads(label, f, got, ref, tol=GRAD_F32):
    """Every parameter gradient within tol x its tensor's largest entry (test_gpu_parity
    test_train_forward_backward_matches_oracle_autograd (c)); parameters the oracle gives no gradient get none."""
    worst = (0.0, "")
    for name, _ in f.named_parameters():
        if "field_output_low" in name:
            continue
        gr, g = ref[name], got[name].detach().double().cpu()
        if gr is None or float(gr.abs().max()) == 0.0:
            assert float(g.abs().max()) <= 1e-12, f"{label} {name}: gradient {float(g.abs().max()):.3e} where fp64 has none"
            continue
        worst = max(worst, (float((g - gr).abs().max()) / float(gr.abs().max()), name))
    print(f"[{label}] parameter gradients: worst error / tensor max {worst[0]:.3e} ({worst[1]}; bound {tol:.0e})")
    assert worst[0] <= tol, f"{label}: parameter gradient {worst[1]} off by {worst[0]:.3e} of its largest entry"


def check_param_grads_bf16(label, f, got, ref):
    """Plain bf16: direction and size per tensor (test_gpu_parity test_reduced_precision_training_bf16_sweeps)."""
    worst_c, worst_r = (0.0, ""), (0.0, "")
    for name, _ in f.named_parameters():
        gr = ref.get(name)
        if "field_output_low" in name or gr is None or float(gr.abs().max()) == 0.0:
            continue
        a, b = got[name].detach().double().cpu().flatten(), gr.flatten()
        assert bool(torch.isfinite(a).all()), f"{label} {name}: non-finite gradient"
        cos = float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))
        worst_c = max(worst_c, (1.0 - cos, name))
        worst_r = max(worst_r, (float((a - b).norm() / (b.norm() + 1e-300)), name))
    print(f"[{label}] parameter gradients: worst 1 - cos {worst_c[0]:.3e} ({worst_c[1]}), worst rel-L2 {worst_r[0]:.3e} "
          f"({worst_r[1]})")
    assert worst_c[0] <= GRAD_BF16_COS, f"{label}: {worst_c[1]}: 1 - cos = {worst_c[0]:.3e}"
    assert worst_r[0] <= GRAD_BF16_REL, f"{label}: {worst_r[1]}: rel-L2 {worst_r[0]:.3e}"


# ---------------------------------------------------------------------------------------------- 2. one training level
# One input set per width, shared by the three MMA modes (the fp64 oracle runs once).  787 x 250 = 196,750 points: 1,538
# tiles of 128 (f32 / bf16x6) or 769 of 256 (bf16) on 256 workgroups; 401 x 250 = 100,250 points: 784 tiles of 128.
LEVEL_CASES = {256: (787, 250, 11), 200: (401, 250, 12)}
_level_cache = {}


def saved_means(f, saved):
    """The contracted sample means a training forward used: the raw-coordinate slots of its saved encoded inputs."""
    lay = f.train_layout()
    assert lay["narrow_dtype"] == torch.float32
    return saved["enc"][:, [lay["enc_map"].index(96 + c) for c in range(3)]]


def _level_case(dev, width):
    if width not in _level_cache:
        R, S, seed = LEVEL_CASES[width]
        f, P, fs = _field(dev, width, seed=seed)
        o, d, pa, eb = _rays(R, S, seed=seed + 100)
        gin = _gin(R * S, seed=seed + 200)
        case = dict(f=f, R=R, S=S, rays=(o.to(dev), d.to(dev), pa.reshape(R).to(dev)), eb=eb.to(dev),
                    gin={k: v.reshape((R, S) + v.shape[1:]).to(dev) for k, v in gin.items()}, gpu={})
        f.set_mma_mode("f32")
        case["means"] = saved_means(f, _run_level(case, "f32")[0]["saved"]).cpu()
        case["ref"], case["gref"], case["dpa"] = oracle_points(P, fs, o, d, pa, eb, gin, case["means"])
        _level_cache[width] = case
    return _level_cache[width]


def _run_level(case, mode):
    """evaluate_frustums_train (analytic normals) -> train_graph._field_backward (input gradient) -> weight gradients."""
    if mode not in case["gpu"]:
        f = case["f"]
        f.set_mma_mode(mode)
        o, d, pa = case["rays"]
        lv = f.evaluate_frustums_train(o, d, pa, case["eb"], want_normals=True)
        go = train_graph._field_backward(f, (o, d, pa), case["eb"], lv, case["gin"], True)
        grads = {k: v.clone() for k, v in weight_grads(f, [(lv["saved"], go, True)]).items()}
        torch.cuda.synchronize()
        case["gpu"][mode] = (lv, go, grads)
    return case["gpu"][mode]


@pytest.mark.parametrize("mode,width", [("f32", 256), ("bf16x6", 256), ("bf16", 256), ("f32", 200)])
def test_training_level_multitile_against_fp64(dev, cus, mode, width):
    """One training level (forward with analytic normals, backward with the input gradient, weight gradients) at a size where
    every workgroup walks >= 3 tiles: every point's outputs and d_input against fp64, the parameter gradients against fp64
    autograd; in the LDS-ring modes every saved row and every layer-gradient row against the exact-fp32 kernels."""
    case = _level_case(dev, width)
    R, S, f = case["R"], case["S"], case["f"]
    N = R * S
    tile = TILE[mode]
    label = f"level {mode} 8x{width}"
    _, grid, _ = multitile_geometry(label, [N], tile, cus)
    lv, go, grads = _run_level(case, mode)
    ref = case["ref"]
    bf16 = mode == "bf16"
    if mode == "bf16x6":  # the oracle ran at the exact kernels' means: the frustum arithmetic is the same fp32 code
        assert torch.equal(saved_means(f, lv["saved"]).cpu(), case["means"])
    for k in ("sigma", "color", "pred_normals", "n_dot_d", "diff", "tint", "roughness"):
        e = point_err(lv[k], ref[k], N)
        if bf16 and k == "sigma":
            e = e / (1.0 + ref[k].abs().reshape(N))
        bound = TOL_BF16 if bf16 else (TOL_UNIT if k in ("pred_normals", "n_dot_d") else TOL)
        check_points(label, k, e, bound, tile, grid)
    # analytic normals: unit vectors through a division by a gradient norm that can be tiny (test_gpu_parity's rule)
    check_normals(label, point_err(lv["normals"], ref["normals"], N), tile, grid, bf16)
    scale = float(case["dpa"].abs().max())
    check_points(label, "d_input / max|d_input|", point_err(go["d_input"], case["dpa"], N) / scale,
                 D_INPUT_BF16 if bf16 else D_INPUT_F32, tile, grid)
    if bf16:
        check_param_grads_bf16(label, f, grads, case["gref"])
    else:
        check_param_grads(label, f, grads, case["gref"])
    if mode == "f32":
        return
    # ring modes: buffer by buffer against the exact-fp32 kernels on the same inputs
    la, ga, _ = _run_level(case, "f32")
    pairs = [("saved." + k, lv["saved"][k], la["saved"][k]) for k in ("bott", "hid", "heads")]
    pairs += [(f"saved.act[{l}]", lv["saved"]["act"][l], la["saved"]["act"][l]) for l in range(8)]
    pairs += [("gout." + k, go[k], ga[k]) for k in ("dz_rgb", "da_mid", "d_bott", "dz_heads", "d_input")]
    pairs += [(f"gout.dy[{l}]", go["dy"][l], ga["dy"][l]) for l in range(8)]
    if not bf16:
        # A hidden unit whose pre-activation sits within rounding of zero can take the other side of a ReLU in the split-bf16
        # sweep than in the exact one; the gradient rows of that point then legitimately differ by O(1) from that unit down.
        # Such points: a saved post-ReLU value exactly zero on one side only.  Their forward rows are held to the bound
        # above; their gradient rows are left out, and there must be few of them.
        flip = torch.zeros(N, dtype=torch.bool, device=lv["saved"]["hid"].device)
        for b, a in [(lv["saved"]["hid"], la["saved"]["hid"])] + [(lv["saved"]["act"][l], la["saved"]["act"][l]) for l in range(8)]:
            flip |= ((b == 0) != (a == 0)).any(dim=1)
        keep = ~flip
        n_flip = int(flip.sum())
        print(f"[{label}] {n_flip} points with a ReLU unit on the other side of zero (left out of the gradient-row comparison)")
        assert n_flip <= N // 1000, f"{label}: {n_flip} points with ReLU units on different sides in the two modes"
    for name, b, a in pairs:
        if not bf16 and name.startswith("gout."):
            b, a = b.reshape(N, -1) if b.dim() < 3 else b.transpose(0, 1), a.reshape(N, -1) if a.dim() < 3 else a.transpose(0, 1)
            b, a = b * keep.reshape(N, *([1] * (b.dim() - 1))), a * keep.reshape(N, *([1] * (a.dim() - 1)))
        if bf16:
            check_points(label, name + " (rel-L2 per tile vs f32)", tile_rel_err(b.reshape(N, -1), a.reshape(N, -1), tile),
                         ROWS_BF16, tile, grid)
        else:  # split bf16 is fp32-equivalent
            sc = max(float(a.abs().max()), 1e-3)
            check_points(label, name + " (vs f32, / tensor max)", point_err(b, a, N) / sc, ROWS_X6, tile, grid)


# ---------------------------------------------------------------------------------------------- 3. multi-job launches
def _zeros(t):
    return {k: (v.zero_() if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def _level_buffers(f, R, S, dev):
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    lv = {"sigma": z(R, S), "color": z(R, S, 3), "pred_normals": z(R, S, 3), "n_dot_d": z(R, S), "diff": z(R, S, 3),
          "tint": z(R, S, 3), "roughness": z(R, S), "raw_density": z(R, S)}
    lv["saved"] = _zeros(f.alloc_saved(R * S, dev))
    return lv


def _fwd_alone(f, job, dev):
    lib = _abi.load_library()
    desc, pk = f.field_desc(), f.packed_weights()
    if job["kind"] == 0:
        o, d, pa, eb = job["rays"]
        R, S = eb.shape[0], eb.shape[1] - 1
        lv = _level_buffers(f, R, S, dev)
        fo, fs = ops.field_outputs_struct(lv), train_graph._saved_struct(lv["saved"])
        check(lib.rsn_field_forward_frustum_train(C.byref(desc), ptr(pk), R, None, S, ptr(o), ptr(d), ptr(pa), ptr(eb),
                                                  C.byref(fo), C.byref(fs), ops._stream()))
        return lv
    dirs, sq = job["inf"]
    M = dirs.shape[0]
    res = {"rgb": torch.zeros(M, 3, device=dev), "saved": _zeros(f.alloc_saved(M, dev))}
    fs = train_graph._saved_struct(res["saved"])
    check(lib.rsn_field_forward_inf_train(C.byref(desc), ptr(pk), M, None, ptr(dirs), ptr(sq), ptr(res["rgb"]), C.byref(fs),
                                          ops._stream()))
    return res


def _fwd_jobs(f, jobs, dev):
    lib = _abi.load_library()
    arr = (_abi.FieldJob * len(jobs))()
    keep, res = [], []
    for q, job in zip(arr, jobs):
        if job["kind"] == 0:
            o, d, pa, eb = job["rays"]
            R, S = eb.shape[0], eb.shape[1] - 1
            lv = _level_buffers(f, R, S, dev)
            fo, fs = ops.field_outputs_struct(lv), train_graph._saved_struct(lv["saved"])
            q.kind, q.n_rays, q.n_samples = 0, R, S
            q.origins, q.directions, q.pixel_area, q.euclid_bins = o.data_ptr(), d.data_ptr(), pa.data_ptr(), eb.data_ptr()
            q.out, q.saved = C.pointer(fo), C.pointer(fs)
            keep += [fo, fs]
            res.append(lv)
        else:
            dirs, sq = job["inf"]
            M = dirs.shape[0]
            r = {"rgb": torch.zeros(M, 3, device=dev), "saved": _zeros(f.alloc_saved(M, dev))}
            fs = train_graph._saved_struct(r["saved"])
            q.kind, q.n_rays, q.n_samples = 1, M, 1
            q.directions, q.sqradius, q.out_rgb = dirs.data_ptr(), sq.data_ptr(), r["rgb"].data_ptr()
            q.saved = C.pointer(fs)
            keep.append(fs)
            res.append(r)
    check(lib.rsn_field_forward_train_jobs(C.byref(f.field_desc()), ptr(f.packed_weights()), len(jobs), arr, ops._stream()))
    torch.cuda.synchronize()
    del keep
    return res


def _gout(f, N, dev):
    g, st = train_graph._alloc_gout(f, N, dev, True)
    _zeros(g)
    return g, st


def _gin_struct(gin):
    gi = FieldGradsIn()
    for k in ("sigma", "color", "pred_normals", "n_dot_d", "roughness"):
        setattr(gi, k, ptr(gin.get(k)))
    return gi


def _bwd_alone(f, job, fwd, dev):
    lib = _abi.load_library()
    desc, pk = f.field_desc(), f.packed_weights()
    if job["kind"] == 0:
        o, d, pa, eb = job["rays"]
        R, S = eb.shape[0], eb.shape[1] - 1
        g, st = _gout(f, R * S, dev)
        gi, fo, fs = _gin_struct(job["gin"]), ops.field_outputs_struct(fwd), train_graph._saved_struct(fwd["saved"])
        check(lib.rsn_field_backward_frustum(C.byref(desc), ptr(pk), R, None, S, ptr(o), ptr(d), ptr(pa), ptr(eb),
                                             C.byref(fo), C.byref(fs), C.byref(gi), C.byref(st), 1, ops._stream()))
        return g
    dirs, sq = job["inf"]
    M = dirs.shape[0]
    g, st = _gout(f, M, dev)
    fs = train_graph._saved_struct(fwd["saved"])
    check(lib.rsn_field_backward_inf(C.byref(desc), ptr(pk), M, None, ptr(dirs), ptr(sq), C.byref(fs), ptr(job["g_rgb"]),
                                     C.byref(st), 1, ops._stream()))
    return g


def _bwd_jobs(f, jobs, fwds, dev):
    lib = _abi.load_library()
    arr = (_abi.FieldBwdJob * len(jobs))()
    keep, res = [], []
    for q, job, fwd in zip(arr, jobs, fwds):
        fs = train_graph._saved_struct(fwd["saved"])
        q.need_input_grad = 1
        if job["kind"] == 0:
            o, d, pa, eb = job["rays"]
            R, S = eb.shape[0], eb.shape[1] - 1
            g, st = _gout(f, R * S, dev)
            gi, fo = _gin_struct(job["gin"]), ops.field_outputs_struct(fwd)
            q.kind, q.n_rays, q.n_samples = 0, R, S
            q.origins, q.directions, q.pixel_area, q.euclid_bins = o.data_ptr(), d.data_ptr(), pa.data_ptr(), eb.data_ptr()
            q.fwd, q.gin = C.pointer(fo), C.pointer(gi)
            keep += [gi, fo]
        else:
            dirs, sq = job["inf"]
            g, st = _gout(f, dirs.shape[0], dev)
            q.kind, q.n_rays, q.n_samples = 1, dirs.shape[0], 1
            q.directions, q.sqradius, q.g_rgb = dirs.data_ptr(), sq.data_ptr(), job["g_rgb"].data_ptr()
        q.saved, q.gout = C.pointer(fs), C.pointer(st)
        keep += [fs, st]
        res.append(g)
    check(lib.rsn_field_backward_jobs(C.byref(f.field_desc()), ptr(f.packed_weights()), len(jobs), arr, ops._stream()))
    torch.cuda.synchronize()
    del keep
    return res


def _inf_inputs(M, seed, dev):
    g = torch.Generator().manual_seed(seed)
    dirs = torch.nn.functional.normalize(torch.randn(M, 3, generator=g), dim=-1)
    sq = 0.01 + torch.rand(M, generator=g) * 0.29  # (kept off 0 for the reason _rays keeps pixel areas >= 1e-4)
    g_rgb = torch.randn(M, 3, generator=g)
    return dirs, sq, g_rgb


def _flat(t, n):
    if t.dim() >= 3 and t.shape[1] == n:  # [L, n, ...]: per-layer rows
        return t.transpose(0, 1).reshape(n, -1)
    return t.reshape(n, -1)


def _assert_bitwise(label, name, a, b, n, tile, grid, base):
    """a, b: buffers of one job ([n, ...] rows, or [L, n, ...] / [L+1, n, ...] per-layer rows)."""
    if torch.equal(a.view(torch.uint8), b.view(torch.uint8)):
        return
    e = (_flat(a, n).double() - _flat(b, n).double()).abs().nan_to_num(float("inf")).amax(dim=1)
    w, i, t, it, e0, e1 = locate(e, tile, grid, base)
    raise AssertionError(f"{label} {name}: the jobs launch differs from the job launched alone: worst {w:.3e} at point {i} "
                         f"(tile {t} of the launch, persistent-loop iteration {it}); iteration 0 {e0:.3e}, iterations >= 1 {e1:.3e}")


@pytest.mark.parametrize("mode", ["f32", "bf16x6", "bf16"])
def test_jobs_launches_equal_separate_launches(dev, cus, mode):
    """rsn_field_forward_train_jobs / rsn_field_backward_jobs with the reflect branch's shape (two frustum levels and a
    get_inf_color job: tb1 and tb2 both live), job boundaries inside a later round and off tile boundaries: every job's outputs,
    saved rows and gradient rows equal the same evaluation launched alone (rsn_field_forward_frustum_train /
    rsn_field_forward_inf_train, rsn_field_backward_frustum / rsn_field_backward_inf) bit for bit -- a tile computes the same
    thing whichever job and iteration it belongs to."""
    tile = TILE[mode]
    k = tile // 128
    f, _, _ = _field(dev, 256, seed=21)
    f.set_mma_mode(mode)
    jobs = []
    for R, S, seed in ((301, 130 * k, 31), (263, 190 * k, 32)):  # 39,130 and 49,970 points per 128 of tile
        o, d, pa, eb = _rays(R, S, seed)
        gin = _gin(R * S, seed + 1)
        jobs.append({"kind": 0, "rays": (o.to(dev), d.to(dev), pa.reshape(R).to(dev), eb.to(dev)),
                     "gin": {kk: v.reshape((R, S) + v.shape[1:]).to(dev) for kk, v in gin.items()}, "n": R * S})
    dirs, sq, g_rgb = _inf_inputs(14000 * k, 33, dev)
    jobs.append({"kind": 1, "inf": (dirs.to(dev), sq.to(dev)), "g_rgb": g_rgb.to(dev), "n": dirs.shape[0]})
    label = f"jobs {mode}"
    _, grid, base = multitile_geometry(label, [j["n"] for j in jobs], tile, cus)
    fj = _fwd_jobs(f, jobs, dev)
    fa = [_fwd_alone(f, j, dev) for j in jobs]
    torch.cuda.synchronize()
    for q, (job, a, b) in enumerate(zip(jobs, fj, fa)):
        for key in [kk for kk in a if kk != "saved"] + ["saved." + kk for kk in a["saved"]]:
            x, y = (a["saved"][key[6:]], b["saved"][key[6:]]) if key.startswith("saved.") else (a[key], b[key])
            _assert_bitwise(label, f"forward job {q} {key}", x, y, job["n"], tile, grid, base[q])
    bj = _bwd_jobs(f, jobs, fj, dev)
    ba = [_bwd_alone(f, j, fwd, dev) for j, fwd in zip(jobs, fa)]
    torch.cuda.synchronize()
    for q, (job, a, b) in enumerate(zip(jobs, bj, ba)):
        for key in a:
            _assert_bitwise(label, f"backward job {q} gout.{key}", a[key], b[key], job["n"], tile, grid, base[q])
    print(f"[{label}] {len(jobs)} jobs (first tiles {base}): forward and backward bit-identical to separate launches")


_inf_cache = {}


@pytest.mark.parametrize("mode", ["f32", "bf16x6", "bf16"])
def test_inf_entry_points_against_fp64(dev, cus, mode):
    """rsn_field_forward_inf_train and rsn_field_backward_inf (get_inf_color in training mode and its backward with the input
    gradient), called directly at 77 rays and at a multi-tile size: colour, parameter gradients (production weight-gradient
    path, no heads) and d loss / d sqradius against fp64 autograd through cpu_ref.inf_color."""
    f, P, fs = _field(dev, 256, seed=41)
    f.set_mma_mode(mode)
    tile = TILE[mode]
    bf16 = mode == "bf16"
    for M in (77, 200003):
        label = f"inf {mode} M={M}"
        dirs, sq, g_rgb = _inf_inputs(M, 42 + M, dev)
        if M > 77:
            _, grid, _ = multitile_geometry(label, [M], tile, cus)
        else:
            grid = 1
        job = {"kind": 1, "inf": (dirs.to(dev), sq.to(dev)), "g_rgb": g_rgb.to(dev)}
        fwd = _fwd_alone(f, job, dev)
        go = _bwd_alone(f, job, fwd, dev)
        grads = weight_grads(f, [(fwd["saved"], go, False)])
        torch.cuda.synchronize()
        if M not in _inf_cache:  # the same parameters and inputs in every mode: one fp64 run
            _inf_cache[M] = oracle_inf(P, fs, dirs, sq, g_rgb)
        rgb, gref, dsq = _inf_cache[M]
        check_points(label, "rgb", point_err(fwd["rgb"], rgb, M), TOL_BF16 if bf16 else INF_F32, tile, grid)
        check_points(label, "d_sqradius / max", point_err(go["d_input"], dsq, M) / float(dsq.abs().max()),
                     D_INPUT_BF16 if bf16 else D_INPUT_F32, tile, grid)
        if bf16:
            check_param_grads_bf16(label, f, grads, gref)
        else:
            check_param_grads(label, f, grads, gref)


# ------------------------------------------------------------------------- 3b. a single call is a one-job launch
# The single entry points and the *_jobs entry points fill the same job block through the same fillers: the same evaluation through
# either must give the same bits in every output, saved buffer and gradient buffer (plain stores only).  Shapes: 5 rays x 29 samples
# = 145 points (two ragged 128-point tiles: exact and bf16x6; one ragged 256-point tile: bf16) with a device-side count of 4 rays in
# buffers for 5, and 37 get_inf_color rays with a device-side count of 33 -- a dropped n_dev shows as rows written by one path only.
ONE_JOB_FIELDS = [("f32", 2, 64), ("bf16", 8, 256), ("bf16x6", 8, 256)]  # the ring kernels serve 8 x 256 only

def _one_job_field(dev, mode, layers, width):
    torch.manual_seed(51)
    f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=layers, base_mlp_layer_width=width).to(dev).train()
    f.set_mma_mode(mode)
    return f


def _one_job_inputs(kind, dev):
    """-> (job as _fwd_alone / _bwd_alone take it, rows per ray count, device-side count tensor, points the count leaves live)."""
    if kind == 0:
        R, S, live = 5, 29, 4
        o, d, pa, eb = _rays(R, S, 52)
        gin = {k: v.reshape((R, S) + v.shape[1:]).to(dev) for k, v in _gin(R * S, 53).items()}
        job = {"kind": 0, "rays": (o.to(dev), d.to(dev), pa.reshape(R).to(dev), eb.to(dev)), "gin": gin, "n": R * S}
        return job, torch.tensor([live], dtype=torch.int32, device=dev), live * S
    dirs, sq, g_rgb = _inf_inputs(37, 54, dev)
    job = {"kind": 1, "inf": (dirs.to(dev), sq.to(dev)), "g_rgb": g_rgb.to(dev), "n": 37}
    return job, torch.tensor([33], dtype=torch.int32, device=dev), 33


def _one_job_forward(f, job, n_dev, dev, as_job):
    """The training forward of `job` through its single entry point, or as a one-job rsn_field_forward_train_jobs launch."""
    lib = _abi.load_library()
    desc, pk = f.field_desc(), f.packed_weights()
    saved = f.alloc_saved(job["n"], dev)
    if job["kind"] == 0:
        o, d, pa, eb = job["rays"]
        R, S = eb.shape[0], eb.shape[1] - 1
        saved["normals"] = torch.empty(R, S, 3, device=dev)
        out = f.alloc_train_level(dev, R, S)
    else:
        dirs, sq = job["inf"]
        out = {"rgb": torch.empty(job["n"], 3, device=dev)}
    _poisoned(out)
    _poisoned(saved)
    fo, fs = ops.field_outputs_struct(out), ops.saved_struct(saved)
    q = _abi.FieldJob()
    q.saved = C.pointer(fs)
    if job["kind"] == 0:
        ops.set_frustum_job(q, R, n_dev, S, o, d, pa, eb)
        q.out = C.pointer(fo)
        single = lambda: lib.rsn_field_forward_frustum_train(  # noqa: E731
            C.byref(desc), ptr(pk), R, ptr(n_dev), S, ptr(o), ptr(d), ptr(pa), ptr(eb), C.byref(fo), C.byref(fs), ops._stream())
    else:
        q.kind, q.n_rays, q.n_dev, q.n_samples = 1, job["n"], n_dev.data_ptr(), 1
        q.directions, q.sqradius, q.out_rgb = dirs.data_ptr(), sq.data_ptr(), out["rgb"].data_ptr()
        single = lambda: lib.rsn_field_forward_inf_train(  # noqa: E731
            C.byref(desc), ptr(pk), job["n"], ptr(n_dev), ptr(dirs), ptr(sq), ptr(out["rgb"]), C.byref(fs), ops._stream())
    check(lib.rsn_field_forward_train_jobs(C.byref(desc), ptr(pk), 1, C.byref(q), ops._stream()) if as_job else single())
    torch.cuda.synchronize()
    return {**out, "saved": saved}


def _one_job_backward(f, job, n_dev, fwd, dev, as_job):
    lib = _abi.load_library()
    desc, pk = f.field_desc(), f.packed_weights()
    g, st = train_graph._alloc_gout(f, job["n"], dev, True)
    _poisoned(g)
    fs = ops.saved_struct(fwd["saved"])
    q = _abi.FieldBwdJob()
    q.need_input_grad, q.saved, q.gout = 1, C.pointer(fs), C.pointer(st)
    if job["kind"] == 0:
        o, d, pa, eb = job["rays"]
        R, S = eb.shape[0], eb.shape[1] - 1
        gi, fo = _gin_struct(job["gin"]), ops.field_outputs_struct(fwd)
        ops.set_frustum_job(q, R, n_dev, S, o, d, pa, eb)
        q.fwd, q.gin = C.pointer(fo), C.pointer(gi)
        single = lambda: lib.rsn_field_backward_frustum(  # noqa: E731
            C.byref(desc), ptr(pk), R, ptr(n_dev), S, ptr(o), ptr(d), ptr(pa), ptr(eb), C.byref(fo), C.byref(fs), C.byref(gi),
            C.byref(st), 1, ops._stream())
    else:
        dirs, sq = job["inf"]
        q.kind, q.n_rays, q.n_dev, q.n_samples = 1, job["n"], n_dev.data_ptr(), 1
        q.directions, q.sqradius, q.g_rgb = dirs.data_ptr(), sq.data_ptr(), job["g_rgb"].data_ptr()
        single = lambda: lib.rsn_field_backward_inf(  # noqa: E731
            C.byref(desc), ptr(pk), job["n"], ptr(n_dev), ptr(dirs), ptr(sq), C.byref(fs), ptr(job["g_rgb"]), C.byref(st), 1,
            ops._stream())
    check(lib.rsn_field_backward_jobs(C.byref(desc), ptr(pk), 1, C.byref(q), ops._stream()) if as_job else single())
    torch.cuda.synchronize()
    return g


def _assert_same_bits(label, a, b, n, live):
    """Buffers of the two paths: equal bit for bit over all n rows, and written (not the fill pattern) in each of the `live` rows."""
    for key in a:
        x, y = a[key], b[key]
        it, pattern = _POISON[x.dtype]
        xb, yb = _flat(x.view(it), n), _flat(y.view(it), n)
        rows = (xb != yb).any(dim=1).nonzero().flatten().tolist()
        assert not rows, f"{label} {key}: the one-job launch differs from the single call in rows {rows[:8]} ({len(rows)} of {n})"
        blank = (xb[:live] == pattern).all(dim=1).nonzero().flatten().tolist()
        assert not blank, f"{label} {key}: rows {blank[:8]} ({len(blank)} of the {live} live rows) were written by neither path"


@pytest.mark.parametrize("mode,layers,width", ONE_JOB_FIELDS)
@pytest.mark.parametrize("kind", [0, 1], ids=["frustum", "inf"])
def test_single_forward_equals_one_job_launch(dev, kind, mode, layers, width):
    """rsn_field_forward_frustum_train / rsn_field_forward_inf_train against rsn_field_forward_train_jobs with that one job (kind 0 / 1)."""
    f = _one_job_field(dev, mode, layers, width)
    job, n_dev, live = _one_job_inputs(kind, dev)
    a, b = (_one_job_forward(f, job, n_dev, dev, as_job) for as_job in (False, True))
    label = f"forward {'inf' if kind else 'frustum'} {mode}"
    _assert_same_bits(label, {k: v for k, v in a.items() if k != "saved"}, b, job["n"], live)
    _assert_same_bits(label + " saved", a["saved"], b["saved"], job["n"], live)


@pytest.mark.parametrize("mode,layers,width", ONE_JOB_FIELDS)
@pytest.mark.parametrize("kind", [0, 1], ids=["frustum", "inf"])
def test_single_backward_equals_one_job_launch(dev, kind, mode, layers, width):
    """rsn_field_backward_frustum / rsn_field_backward_inf against rsn_field_backward_jobs with that one job (kind 0 / 1), both on
    the saved buffers of one training forward, with the input gradient."""
    f = _one_job_field(dev, mode, layers, width)
    job, n_dev, live = _one_job_inputs(kind, dev)
    fwd = _one_job_forward(f, job, n_dev, dev, as_job=False)
    a, b = (_one_job_backward(f, job, n_dev, fwd, dev, as_job) for as_job in (False, True))
    _assert_same_bits(f"backward {'inf' if kind else 'frustum'} {mode} gout", a, b, job["n"], live)


def test_weight_grads_leave_no_mode_behind(dev):
    """train_graph._weight_grads passes its mode and its order of addition to every call it makes and leaves the module's defaults
    alone: after the weight gradients of a plain-bf16 field with the ordered reduction, _WGRAD_MODE / _WGRAD_ORDERED are still 0 /
    False, and a bare _wgrad_multi call is the exact-fp32 reduction -- within 2e-5 x max|ref| of the fp64 product of the unrounded
    operands (test_gpu_parity.test_weight_grad_segments_and_shapes' bound), which bf16 operands (2^-9 each) miss by far."""
    f = _one_job_field(dev, "bf16", 8, 256)
    job, _, _ = _one_job_inputs(0, dev)
    o, d, pa, eb = job["rays"]
    lv = f.evaluate_frustums_train(o, d, pa, eb, want_normals=True)
    go = train_graph._field_backward(f, (o, d, pa), eb, lv, job["gin"], True)
    acc = train_graph._GradAcc(f)
    train_graph._weight_grads(f, [(lv["saved"], go, True)], acc, ordered=True)
    grads = acc.finish()
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and float(grads["mlp_base.layers.3.weight"].abs().max()) > 0.0
    assert train_graph._WGRAD_MODE == 0 and train_graph._WGRAD_ORDERED is False
    g = torch.Generator().manual_seed(64)
    dy, x = torch.randn(300, 64, generator=g), torch.randn(300, 64, generator=g)
    ref = dy.double().t() @ x.double()
    dw = torch.zeros(64, 64, device=dev)
    train_graph._wgrad_multi([(dy.to(dev), x.to(dev))], 64, 64, dw, 0, None)
    err, bound = float((dw.double().cpu() - ref).abs().max()), 2e-5 * float(ref.abs().max())
    print(f"bare _wgrad_multi after a bf16 ordered step: dW err {err:.3e} / bound {bound:.3e}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------- 4. whole steps
def _weighted_loss(out, tgt, wr):
    """_loss_from_outputs of test_gpu_parity with a weight per ray instead of the mean over rays."""
    loss = 0.0
    for k in ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine"):
        loss = loss + (wr[:, None] * (out[k] - tgt[k]) ** 2).sum()
    for lvl, c1, c2 in (("coarse", 3e-3, 1e-2), ("fine", 3e-3, 1e-1)):
        w = out[f"weights_{lvl}"].detach() * wr[:, None, None]
        loss = loss + c1 * torch.sum(w * torch.sum((out[f"normals_{lvl}"].detach() - out[f"pred_normals_{lvl}"]) ** 2,
                                                   dim=-1, keepdim=True))
        loss = loss + c2 * torch.sum(w * torch.clamp(out[f"n_dot_d_{lvl}"], min=0.0) ** 2)
    return loss


def _round_end_rays(n_points, S, tile, grid, base=0, first_index=0):
    """Rays (of S samples) with points in the last tile of every round of a launch whose tiles from `base` on hold these
    points, and in its last tile: the first and the last ray of each such tile."""
    n_tiles = base + -(-n_points // tile)
    ends = sorted({t for t in range(grid - 1, n_tiles, grid) if t >= base} | {n_tiles - 1})
    rays = set()
    for t in ends:
        p0, p1 = (t - base) * tile, min(n_points, (t - base + 1) * tile) - 1
        rays |= {first_index + p0 // S, first_index + p1 // S}
    return rays


@pytest.mark.parametrize("mode,samples", [("f32", (128, 128, 64, 64)), ("bf16x6", (128, 128, 64, 64)),
                                          ("f32", (64, 128, 64, 64))])
def test_whole_step_against_fp64_on_a_ray_subset(dev, cus, mode, samples):
    """The headline step (4096 rays x 128/128/64/64, 8 x 256) and BASELINE configs[2] (64/128/64/64): one training forward and
    backward, the oracle in fp64 at the sample positions the kernels used (bins + contracted means, as test_gpu_parity's
    test_train_forward_backward_matches_oracle_autograd (c)).  The loss weights ~256 rays -- the first and last, rays in the
    last tile of every round of each level, a seeded random sample -- and zero elsewhere: those rays still run through every
    kernel, so junk written for them shows in the parameter gradients."""
    R, tile = 4096, TILE[mode]
    torch.manual_seed(0)
    model = pkg.ReflectSamplingNeRFModelConfig(
        num_coarse_samples=samples[0], num_importance_samples=samples[1], num_reflect_coarse_samples=samples[2],
        num_reflect_importance_samples=samples[3]).setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 2.0
    P = {k: v.detach().clone() for k, v in model.field.state_dict().items()}
    model.to(dev).train()
    model.field.set_mma_mode(mode)
    o, d, pa = cpu_ref.synthetic_rays(R, seed=5)
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev), nears=nears.to(dev),
                       fars=fars.to(dev))
    label = f"step {mode} {R}x{samples}"
    for lvl, S in (("coarse", samples[0]), ("fine", samples[1])):  # the BASELINE sizes: full tiles, whole rounds
        multitile_geometry(f"{label} {lvl}", [R * S], tile, cus, fixed_size=True)
    torch.manual_seed(9)
    model._keep_train_state = True
    try:
        out = model._get_outputs_train(rb)
        st = model._train_state
    finally:
        model._keep_train_state, model._train_state = False, None
    M = st["M"]
    mask = out["mask"].cpu()
    assert 0 < M < R and int(mask.sum()) == M
    ray_index = st["rs"]["ray_index"][:M].long().cpu()
    # ---- the ray subset
    grid_p = lambda n: min(-(-n // tile), cus)  # noqa: E731
    sub = {0, R - 1}
    for S in samples[:2]:
        sub |= _round_end_rays(R * S, S, tile, grid_p(R * S))
    comp = set()  # compacted indices of reflected rays: reflect-coarse + get_inf_color (one launch), reflect-fine
    tiles_rc = -(-M * samples[2] // tile)
    g_rc = min(tiles_rc + -(-M // tile), cus)
    comp |= _round_end_rays(M * samples[2], samples[2], tile, g_rc)
    comp |= _round_end_rays(M, 1, tile, g_rc, base=tiles_rc)
    comp |= _round_end_rays(M * samples[3], samples[3], tile, grid_p(M * samples[3]))
    print(f"[{label}] M = {M} reflected rays: reflect-coarse + inf launch {tiles_rc + -(-M // tile)} tiles on {g_rc} "
          f"workgroups, reflect-fine {-(-M * samples[3] // tile)} tiles")
    sub |= {int(ray_index[i]) for i in comp}
    # rays whose reflect-mask inputs (model.py:229: accumulation > 1e-2 and n.d < 0) sit within rounding of a threshold could
    # take the other branch in fp64: they stay out of the subset, so that the oracle's mask is the kernels' on every ray
    acc_f = out["accumulation_fine"].reshape(R).double().cpu()
    ndd = (st["cf"]["normals"].double().cpu() * d.double()).sum(-1)
    edge = ((acc_f - 1e-2).abs() <= 1e-5) | (ndd.abs() <= 1e-5)
    sub = {r for r in sub if not bool(edge[r])}
    g = torch.Generator().manual_seed(77)
    for r in torch.randperm(R, generator=g).tolist():
        if len(sub) >= 256:
            break
        if not bool(edge[r]):
            sub.add(r)
    sub = torch.tensor(sorted(sub))
    n = sub.numel()
    wr = torch.zeros(R, dtype=torch.float64)
    wr[sub] = 0.5 + torch.rand(n, generator=g, dtype=torch.float64)
    tgt = {k: torch.rand(R, 3, generator=g) for k in ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse",
                                                      "mid_reflect_fine")}
    # ---- the oracle on the subset, at the kernels' sample positions, in fp64
    inv = torch.full((R,), -1, dtype=torch.long)
    inv[ray_index] = torch.arange(M)
    rrows = inv[sub[mask[sub]]]  # compacted rows of the subset's reflected rays, in ray order
    bins, means = {}, {}
    for name, sbk, ebk, lvk, S, rows in (("coarse", "sb_c", "eb_c", "lc", samples[0], sub),
                                         ("fine", "sb_f", "eb_f", "lf", samples[1], sub),
                                         ("reflect_coarse", "sb_rc", "eb_rc", "lrc", samples[2], rrows),
                                         ("reflect_fine", "sb_rf", "eb_rf", "lrf", samples[3], rrows)):
        bins[name + "_spacing"] = st[sbk].cpu()[rows].double()
        bins[name + "_euclid"] = st[ebk].cpu()[rows].double()
        means[name] = saved_means(model.field, st[lvk]["saved"]).reshape(-1, S, 3).cpu()[rows].double()
    fs, ms = cpu_ref.FieldSpec(num_layers=8, width=256), cpu_ref.ModelSpec(*samples)
    with default_dtype(torch.float64):
        P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
        jit = {k: torch.zeros(n, s + 1) for k, s in zip(("coarse", "fine", "reflect_coarse", "reflect_fine"), samples)}
        ref = cpu_ref.get_outputs(P64, fs, ms, o[sub].double(), d[sub].double(), pa[sub].double(), nears[sub].double(),
                                  fars[sub].double(), training=True, jitter=jit, bins=bins, means=means)
        assert torch.equal(ref["mask"], mask[sub]), f"{label}: the fp64 reflect mask differs from the kernels' on the subset"
        _weighted_loss(ref, {k: v[sub].double() for k, v in tgt.items()}, wr[sub]).backward()
    # ---- the HIP backward of the same loss (analytic normals: the oracle's on the subset -- a detached target)
    checked = dict(out)
    for lvl in ("coarse", "fine"):
        nr = out[f"normals_{lvl}"].detach().clone()
        nr[sub.to(dev)] = ref[f"normals_{lvl}"].float().to(dev)
        checked[f"normals_{lvl}"] = nr
    _weighted_loss(checked, {k: v.to(dev) for k, v in tgt.items()}, wr.float().to(dev)).backward()
    torch.cuda.synchronize()
    # ---- forward values of the subset
    for k in ("mid_rgb_coarse", "mid_rgb_fine", "mid_reflect_coarse", "mid_reflect_fine", "accumulation_coarse",
              "accumulation_fine", "weights_coarse", "weights_fine", "diff", "tint", "roughness", "pred_normals_coarse",
              "pred_normals_fine", "n_dot_d_coarse", "n_dot_d_fine"):
        e = point_err(out[k][sub.to(dev)], ref[k], n)
        bound = TOL_UNIT if k.startswith(("pred_normals", "n_dot_d")) else TOL
        w, i, _, _, _, _ = locate(e, 1, 1)
        print(f"[{label}] {k}: worst {w:.3e} (bound {bound:.0e}) at ray {int(sub[i])}")
        assert w <= bound, f"{label} {k}: {w:.3e} at ray {int(sub[i])}"
    for lvl in ("coarse", "fine"):
        e = point_err(out[f"normals_{lvl}"][sub.to(dev)], ref[f"normals_{lvl}"], n * samples[lvl == "fine"])
        check_normals(f"{label} {lvl} (subset)", e, samples[lvl == "fine"], 1)
    got = {name: p.grad for name, p in model.field.named_parameters() if p.grad is not None}
    check_param_grads(label, model.field, got, _param_grads_fp64(P64), GRAD_STEP)


def test_config3_bf16_eval_all_rays(dev, cus):
    """BASELINE configs[3] (16384 rays x 192 samples, 8 x 256, plain-bf16 eval on the LDS ring): every ray against the
    exact-fp32 kernel within the bf16 tolerance, and a strided subset that includes the last ray against fp64."""
    from reflect_sampling_nerf_amd._abi import RSN_SPACING_UNIFORM

    R, S = 16384, 192
    f, P, fs = _field(dev, 256, seed=0)
    f.eval()
    o, d, pa = cpu_ref.synthetic_rays(R, seed=0)
    od, dd, pad = o.to(dev), d.to(dev), pa.reshape(R).to(dev)
    nears, fars = torch.full((R,), 2.0, device=dev), torch.full((R,), 6.0, device=dev)
    _, eb = ops.sample_spaced(R, None, S, RSN_SPACING_UNIFORM, 1.0, nears, fars, None)
    label = "configs[3] bf16 eval"
    _, grid, _ = multitile_geometry(label, [R * S], 256, cus, fixed_size=True)  # 12,288 full 256-point tiles
    f.set_mma_mode("bf16")
    lv = f.evaluate_frustums(od, dd, pad, eb)
    f.set_mma_mode("f32")
    ref = f.evaluate_frustums(od, dd, pad, eb)
    torch.cuda.synchronize()
    N = R * S
    check_points(label, "color vs f32 kernel", point_err(lv["color"], ref["color"], N), TOL_BF16, 256, grid)
    check_points(label, "sigma vs f32 kernel (/ (1 + |sigma|))",
                 point_err(lv["sigma"], ref["sigma"], N) / (1.0 + ref["sigma"].double().abs().cpu().reshape(N)),
                 TOL_BF16, 256, grid)
    rows = torch.cat([torch.arange(0, R, 128), torch.tensor([R - 1])])
    with torch.no_grad(), default_dtype(torch.float64):
        P64 = {k: v.double() for k, v in P.items()}
        r64 = cpu_ref.field_level(P64, fs, o[rows].double(), d[rows].double(), pa[rows].double(), eb.cpu()[rows].double(),
                                  training=False, want_normals=False)
    pts = (rows[:, None] * S + torch.arange(S)).reshape(-1)
    n = rows.numel() * S
    spread = lambda e: torch.zeros(N, dtype=torch.float64).index_put_((pts,), e)  # noqa: E731  (errors at their points)
    check_points(label, "color vs fp64", spread(point_err(lv["color"][rows.to(dev)], r64["color"], n)), CFG3_FP64, 256, grid)
    e = point_err(lv["sigma"][rows.to(dev)], r64["sigma"], n) / (1.0 + r64["sigma"].abs().reshape(n))
    check_points(label, "sigma vs fp64 (/ (1 + |sigma|))", spread(e), TOL_BF16, 256, grid)
