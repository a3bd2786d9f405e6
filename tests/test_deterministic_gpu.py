"""Ordered weight-gradient reduction (ABI 18: rsn_weight_grad_multi_dev_ordered / rsn_weight_grad_jobs_ordered) and the deterministic
training step built on it (Model.set_deterministic): the sums of the atomic path within the same fp64 bound, and the SAME BITS on every
repeat whatever the workspace held before.  Kernel-level tests call the C ABI through ctypes with a torch-allocated workspace."""
import ctypes as C
import functools

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi

pytestmark = pytest.mark.gpu

MODES = {"f32": _abi.RSN_MMA_F32, "bf16x6": _abi.RSN_MMA_BF16X6, "bf16": _abi.RSN_MMA_BF16}
BOUND = 2e-5  # x max|ref|: the atomic path's bound in test_gpu_parity (test_weight_grad_segments_and_shapes and its kin)
LENS = [1000, 0, 37, 5003, 3]
SHAPES = [  # test_weight_grad_segments_and_shapes: n_out, k_in, ld_dy, ld_x
    (256, 256, 256, 256), (256, 104, 256, 104), (128, 40, 128, 40), (16, 256, 16, 256), (3, 128, 4, 128), (250, 99, 251, 99),
    (37, 130, 38, 132)]
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


def _ws_bytes(segs, n_jobs, n_out, k_in, mode):
    lib = pkg.load_library()
    segs = [sg for sg in segs if sg[0].shape[0] > 0]
    npts = (C.c_int64 * len(segs))(*[sg[0].shape[0] for sg in segs])
    op = (1 if segs[0][1].dtype == BF else 0) | (2 if segs[0][0].dtype == BF else 0)
    need = int(lib.rsn_weight_grad_workspace_bytes(len(segs), npts, n_jobs, n_out, k_in, mode, op))
    assert need > 0, lib.rsn_last_error()
    return need


def _workspace(dev, nbytes, fill=None):
    ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    if fill is not None:
        ws.fill_(fill)
    return ws


def _segment_args(segs):
    ns = len(segs)
    npts = (C.c_int64 * ns)(*[sg[0].shape[0] for sg in segs])
    cnt = [sg[2] if len(sg) > 2 else None for sg in segs]
    ndev = (C.c_void_p * ns)(*[None if c is None else c[0].data_ptr() for c in cnt])
    per = (C.c_int32 * ns)(*[1 if c is None else int(c[1]) for c in cnt])
    return ns, npts, ndev, per


def ordered_multi(segs, n_out, k_in, dw, col0, db, mode, ws=None, ws_bytes=None, col_map=None):
    """rsn_weight_grad_multi_dev_ordered on segs = [(dy, x[, (device count, rows per count)])]; -> return code."""
    lib = pkg.load_library()
    segs = [sg for sg in segs if sg[0].shape[0] > 0]
    ns, npts, ndev, per = _segment_args(segs)
    dys = (C.c_void_p * ns)(*[sg[0].data_ptr() for sg in segs])
    xs = (C.c_void_p * ns)(*[sg[1].data_ptr() for sg in segs])
    op = (1 if segs[0][1].dtype == BF else 0) | (2 if segs[0][0].dtype == BF else 0)
    if ws is None:
        ws = _workspace(dw.device, _ws_bytes(segs, 1, n_out, k_in, mode))
    nbytes = ws.numel() * 4 if ws_bytes is None else ws_bytes
    return lib.rsn_weight_grad_multi_dev_ordered(
        ns, npts, ndev, per, dys, segs[0][0].stride(0), n_out, xs, segs[0][1].stride(0), k_in, _abi.ptr(col_map),
        C.c_void_p(dw.data_ptr() + 4 * col0), dw.stride(0), _abi.ptr(db), mode, op, _abi.ptr(ws), nbytes,
        torch.cuda.current_stream().cuda_stream)


def ordered_jobs(jobs, n_out, k_in, mode, ws):
    """rsn_weight_grad_jobs_ordered on jobs = [(segs, dw, col0, db, col_map)]; -> return code."""
    lib = pkg.load_library()
    ns, npts, ndev, per = _segment_args(jobs[0][0])
    arr = (_abi.WGradJob * len(jobs))()
    hold = []
    for q, (segs, dw, c0, db, cmap) in zip(arr, jobs):
        dys = (C.c_void_p * ns)(*[sg[0].data_ptr() for sg in segs])
        xs = (C.c_void_p * ns)(*[sg[1].data_ptr() for sg in segs])
        hold += [dys, xs]
        q.dy, q.x = dys, xs
        q.col_map = None if cmap is None else cmap.data_ptr()
        q.dw, q.ld_dw = dw.data_ptr() + 4 * c0, dw.stride(0)
        q.db = None if db is None else db.data_ptr()
    ref = jobs[0][0]
    return lib.rsn_weight_grad_jobs_ordered(ns, npts, ndev, per, len(jobs), arr, ref[0][0].stride(0), n_out, ref[0][1].stride(0), k_in,
                                            mode, 0, _abi.ptr(ws), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max())


@functools.lru_cache(maxsize=None)
def _shape_case(n_out, k_in, ld_dy, ld_x):
    """Operands of one shape (host), and the fp64 products of the exact and of the bf16-rounded operands: computed once, shared."""
    g = torch.Generator().manual_seed(n_out * 1000 + k_in)
    segs, ref = [], {"w": 0, "b": 0, "w_bf": 0, "w0": None, "w0_bf": None}
    for n in LENS:
        dy, x = torch.randn(n, ld_dy, generator=g), torch.randn(n, ld_x, generator=g)
        a, b = dy[:, :n_out], x[:, :k_in]
        w, w_bf = a.double().t() @ b.double(), a.bfloat16().double().t() @ b.bfloat16().double()
        if ref["w0"] is None:
            ref["w0"], ref["w0_bf"] = w, w_bf
        ref["w"], ref["w_bf"], ref["b"] = ref["w"] + w, ref["w_bf"] + w_bf, ref["b"] + a.double().sum(0)
        segs.append((dy, x))
    return segs, ref


@pytest.mark.parametrize("mode", ["f32", "bf16x6", "bf16"])
@pytest.mark.parametrize("n_out,k_in,ld_dy,ld_x", SHAPES)
def test_ordered_weight_grad_shapes_accuracy_repeat_accumulate(dev, n_out, k_in, ld_dy, ld_x, mode):
    """Every launcher variant (row-block splits P = 1, 2, 4; NKB 2, 4, 8; vector and scalar loads; fp32, split-bf16, bf16) over
    segments with an empty one, one below a pipeline stage and ragged ones: ~757 stages on dozens of workgroups.
    Accuracy: the atomic path's bound, 2e-5 max|ref|, against the fp64 product (plain bf16 on its vector path: of the bf16-rounded
    operands, as test_weight_grad_mma_modes).  Repeat: three calls into zeroed outputs -- fresh, NaN-filled and 1e30-filled workspace
    -- give equal bits and nothing non-finite.  Accumulation: a second call (first segment, no bias) into the non-zero dW at column
    offset 5 of a k_in + 5 wide matrix adds its product and leaves columns [:5] exactly 0."""
    host, ref = _shape_case(n_out, k_in, ld_dy, ld_x)
    segs = [(dy.to(dev), x.to(dev)) for dy, x in host]
    m = MODES[mode]
    vector_path = n_out > 32 and k_in % (8 if k_in > 128 else 4 if k_in > 64 else 2) == 0
    rounded = mode == "bf16" and vector_path
    ref_w, ref_w0 = (ref["w_bf"], ref["w0_bf"]) if rounded else (ref["w"], ref["w0"])
    need = _ws_bytes(segs, 1, n_out, k_in, m)
    outs = []
    for fill in (None, float("nan"), 1e30):
        dw, db = torch.zeros(n_out, k_in + 5, device=dev), torch.zeros(n_out, device=dev)
        assert ordered_multi(segs, n_out, k_in, dw, 5, db, m, _workspace(dev, need, fill)) == 0, pkg.load_library().rsn_last_error()
        outs.append((dw, db))
    dw, db = outs[0]
    e_w, e_b = _err(dw[:, 5:], ref_w), _err(db, ref["b"])
    print(f"ordered {mode} {n_out}x{k_in}: dW err {e_w:.3e} / bound {BOUND * float(ref_w.abs().max()):.3e}, "
          f"db err {e_b:.3e} / bound {BOUND * float(ref['b'].abs().max()):.3e}, workspace {need} B")
    for dw2, db2 in outs[1:]:
        assert torch.equal(dw2, dw) and torch.equal(db2, db), "the result depends on the run or on the workspace's old contents"
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    assert e_w <= BOUND * float(ref_w.abs().max())
    assert e_b <= BOUND * float(ref["b"].abs().max())
    assert float(dw[:, :5].abs().max()) == 0.0
    db_before = db.clone()
    assert ordered_multi(segs[:1], n_out, k_in, dw, 5, None, m, _workspace(dev, need, float("nan"))) == 0
    assert _err(dw[:, 5:], ref_w + ref_w0) <= BOUND * float(ref_w.abs().max())
    assert float(dw[:, :5].abs().max()) == 0.0 and torch.equal(db, db_before)


@pytest.mark.parametrize("n_out,k_in,x_bf16,dy_bf16", [(256, 256, True, True), (256, 104, False, True), (128, 40, False, True),
                                                       (128, 256, True, True), (16, 256, True, False), (3, 128, True, False),
                                                       (64, 64, True, True), (256, 128, True, True)])
def test_ordered_weight_grad_bf16_rows(dev, n_out, k_in, x_bf16, dy_bf16):
    """The operand combinations of test_weight_grad_bf16_rows (rows that ARE bf16 in memory, one segment cut by a device-side
    count) through the ordered call: its bound against the fp64 product of the bf16 values, and equal bits on a repeat with a
    NaN-filled workspace."""
    g = torch.Generator().manual_seed(7 * n_out + k_in)
    lens = [1000, 37, 5003, 640]
    count = torch.tensor([9], dtype=torch.int32, device=dev)  # the last segment holds 9 x 64 = 576 of its 640 rows
    segs = []
    ref_w, ref_b = torch.zeros(n_out, k_in, dtype=torch.float64), torch.zeros(n_out, dtype=torch.float64)
    for si, n in enumerate(lens):
        dy, x = torch.randn(n, n_out, generator=g), torch.randn(n, k_in, generator=g)
        ld_dy = n_out + (n_out & 1) if n_out > 32 else (16 if n_out > 4 else 4)
        dyp = torch.zeros(n, ld_dy)
        dyp[:, :n_out] = dy
        dyd = dyp.to(dev).bfloat16() if dy_bf16 else dyp.to(dev)
        xd = x.to(dev).bfloat16() if x_bf16 else x.to(dev)
        live = 576 if si == 3 else n
        ref_w += dyd[:live, :n_out].bfloat16().double().cpu().t() @ xd[:live].bfloat16().double().cpu()
        ref_b += dyd[:live, :n_out].double().cpu().sum(0)
        segs.append((dyd, xd, (count, 64)) if si == 3 else (dyd, xd))
    need = _ws_bytes(segs, 1, n_out, k_in, MODES["bf16"])
    outs = []
    for fill in (None, float("nan")):
        dw, db = torch.zeros(n_out, k_in, device=dev), torch.zeros(n_out, device=dev)
        assert ordered_multi(segs, n_out, k_in, dw, 0, db, MODES["bf16"], _workspace(dev, need, fill)) == 0, \
            pkg.load_library().rsn_last_error()
        outs.append((dw, db))
    (dw, db), (dw2, db2) = outs
    print(f"ordered bf16 rows {n_out}x{k_in}: dW err {_err(dw, ref_w):.3e} / {BOUND * float(ref_w.abs().max()):.3e}, "
          f"db err {_err(db, ref_b):.3e} / {BOUND * float(ref_b.abs().max()):.3e}")
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert _err(dw, ref_w) <= BOUND * float(ref_w.abs().max())
    assert _err(db, ref_b) <= BOUND * float(ref_b.abs().max())


@pytest.mark.parametrize("mode,n_out,k_in", [("f32", 256, 256), ("bf16x6", 256, 256), ("bf16", 256, 256), ("f32", 16, 256),
                                             ("f32", 250, 99)])
def test_ordered_weight_grad_empty_slots(dev, mode, n_out, k_in):
    """Most wave slots idle: a segment sized for 6043 rows whose DEVICE-side count leaves 40 (5 fp32 stages against dozens of wave
    slots) and a segment whose count is 0.  The reducer must take the live slots only -- the fp64 product over the 40 live rows
    within the bound, equal bits with a NaN-filled workspace -- and with every count 0, dW and db keep their bits (-0.0 included)."""
    g = torch.Generator().manual_seed(n_out + 3 * k_in)
    ld_dy = n_out + (n_out & 1)
    dy, x = torch.randn(6043, ld_dy, generator=g), torch.randn(6043, k_in, generator=g)
    dy2, x2 = torch.randn(500, ld_dy, generator=g), torch.randn(500, k_in, generator=g)
    c40, c0 = torch.tensor([40], dtype=torch.int32, device=dev), torch.tensor([0], dtype=torch.int32, device=dev)
    m = MODES[mode]
    a, b = dy[:40, :n_out], x[:40]
    rounded = mode == "bf16" and n_out > 32 and k_in % 8 == 0
    ref_w = a.bfloat16().double().t() @ b.bfloat16().double() if rounded else a.double().t() @ b.double()
    ref_b = a.double().sum(0)
    segs = [(dy.to(dev), x.to(dev), (c40, 1)), (dy2.to(dev), x2.to(dev), (c0, 1))]
    need = _ws_bytes(segs, 1, n_out, k_in, m)
    outs = []
    for fill in (None, float("nan")):
        dw, db = torch.zeros(n_out, k_in, device=dev), torch.zeros(n_out, device=dev)
        assert ordered_multi(segs, n_out, k_in, dw, 0, db, m, _workspace(dev, need, fill)) == 0
        outs.append((dw, db))
    (dw, db), (dw2, db2) = outs
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    assert _err(dw, ref_w) <= BOUND * float(ref_w.abs().max())
    assert _err(db, ref_b) <= BOUND * float(ref_b.abs().max())
    # every count 0: nothing is added, not even +0.0
    segs0 = [(segs[0][0], segs[0][1], (c0, 1)), segs[1]]
    dw0 = torch.randn(n_out, k_in, generator=g).to(dev)
    dw0[0, :8] = -0.0
    db0 = torch.randn(n_out, generator=g).to(dev)
    db0[0] = -0.0
    keep_w, keep_b = dw0.clone(), db0.clone()
    assert ordered_multi(segs0, n_out, k_in, dw0, 0, db0, m, _workspace(dev, need, float("nan"))) == 0
    assert torch.equal(dw0.view(torch.int32), keep_w.view(torch.int32)) and torch.equal(db0.view(torch.int32), keep_b.view(torch.int32))


@pytest.mark.parametrize("mode", ["f32", "bf16x6"])
@pytest.mark.parametrize("n_jobs,n_out,k_in", [(2, 256, 256), (5, 256, 256), (2, 256, 104)])
def test_ordered_weight_grad_jobs_equal_single_job_calls(dev, mode, n_jobs, n_out, k_in):
    """rsn_weight_grad_jobs_ordered against rsn_weight_grad_multi_dev_ordered, job by job, each into its own output.
    From the code (wgrad_launch / wgrad_grid): workgroups per job = min(round(sqrt(stages t_stage / (nsub t_flush))), CUs / n_jobs), and
    a job's wave slots, their stages and the reducer's order depend on that number alone.  The segments here (about 173 fp32 stages)
    put the square root at <= 40, below 256 CUs / 5, so on an MI355X the per-job grid is the SAME in both calls and the results must
    be BITWISE equal.  The test reads the fact off the workspace sizes (4 slots per workgroup: bytes(n_jobs) == n_jobs * bytes(1)
    exactly when the per-job grids agree); on a device with so few CUs that the cap bites, it compares within the fp64 bound
    instead.  Both calls are also held to the bound against fp64.  Job 1 lands at a column offset without bias; the 104-column
    shape goes through a column map."""
    g = torch.Generator().manual_seed(31 * n_jobs + k_in)
    lens = [700, 0, 33, 640]
    count = torch.tensor([7], dtype=torch.int32, device=dev)  # the last segment holds 7 x 64 = 448 of its 640 rows
    cmap = torch.randperm(k_in, generator=g).to(torch.int32).to(dev) if k_in == 104 else None
    m = MODES[mode]
    jobs, singles, refs = [], [], []
    for jb in range(n_jobs):
        segs, ref_w, ref_b = [], torch.zeros(n_out, k_in, dtype=torch.float64), torch.zeros(n_out, dtype=torch.float64)
        for si, n in enumerate(lens):
            if n == 0:
                continue
            dy, x = torch.randn(n, n_out, generator=g), torch.randn(n, k_in, generator=g)
            live = 448 if si == 3 else n
            ref_w += dy[:live].double().t() @ x[:live].double()
            ref_b += dy[:live].double().sum(0)
            segs.append((dy.to(dev), x.to(dev), (count, 64)) if si == 3 else (dy.to(dev), x.to(dev)))
        c0 = 5 if jb == 1 else 0
        mk = lambda: (torch.zeros(n_out, k_in + c0, device=dev), None if jb == 1 else torch.zeros(n_out, device=dev))  # noqa: E731
        dw, db = mk()
        jobs.append((segs, dw, c0, db, cmap))
        singles.append(mk())
        refs.append((ref_w, ref_b))
    b1, bn = _ws_bytes(jobs[0][0], 1, n_out, k_in, m), _ws_bytes(jobs[0][0], n_jobs, n_out, k_in, m)
    same_grid = bn == n_jobs * b1
    assert ordered_jobs(jobs, n_out, k_in, m, _workspace(dev, bn, float("nan"))) == 0, pkg.load_library().rsn_last_error()
    for (segs, dw, c0, db, _), (dw1, db1), (ref_w, ref_b) in zip(jobs, singles, refs):
        assert ordered_multi(segs, n_out, k_in, dw1, c0, db1, m, _workspace(dev, b1, 1e30), col_map=cmap) == 0
        exp = ref_w
        if cmap is not None:
            exp = torch.zeros_like(ref_w)
            exp[:, cmap.cpu().long()] = ref_w
        for got_w, got_b in ((dw, db), (dw1, db1)):
            assert _err(got_w[:, c0:], exp) <= BOUND * float(ref_w.abs().max())
            assert got_b is None or _err(got_b, ref_b) <= BOUND * float(ref_b.abs().max())
            assert c0 == 0 or float(got_w[:, :c0].abs().max()) == 0.0
        if same_grid:
            assert torch.equal(dw, dw1) and (db is None or torch.equal(db, db1))
    print(f"jobs {n_jobs} x {n_out}x{k_in} {mode}: per-job grid equal to the single-job call's: {same_grid}")


def test_ordered_weight_grad_workspace_too_small(dev):
    """A workspace one byte short: RSN_ERR_INVALID_ARGUMENT before any launch, the needed size in rsn_last_error(), outputs untouched."""
    host, _ = _shape_case(256, 104, 256, 104)
    segs = [(dy.to(dev), x.to(dev)) for dy, x in host]
    need = _ws_bytes(segs, 1, 256, 104, 0)
    ws = _workspace(dev, need)
    dw, db = torch.full((256, 104), 3.0, device=dev), torch.full((256,), -2.0, device=dev)
    rc = ordered_multi(segs, 256, 104, dw, 0, db, 0, ws, ws_bytes=need - 1)
    msg = pkg.load_library().rsn_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1 and str(need) in msg, (rc, msg)
    assert bool((dw == 3.0).all()) and bool((db == -2.0).all())
    jobs = [(segs, dw, 0, db, None), (segs, dw.clone(), 0, None, None)]
    small = _workspace(dev, _ws_bytes(segs, 2, 256, 104, 0) - 4)
    assert ordered_jobs(jobs, 256, 104, 0, small) == -1 and "needs" in pkg.load_library().rsn_last_error().decode()
    torch.cuda.synchronize()
    assert bool((dw == 3.0).all()) and bool((db == -2.0).all())


# ---------------------------------------------------------------------------------------------- whole training steps
def _train_setup(dev, R, samples, layers, width, mma, deterministic, seed=0):
    """test_gpu_parity._train_setup (the setup of test_weight_grad_groups_two_equals_one)."""
    torch.manual_seed(seed)
    cfg = pkg.ReflectSamplingNeRFModelConfig(num_coarse_samples=samples[0], num_importance_samples=samples[1],
                                            num_reflect_coarse_samples=samples[2], num_reflect_importance_samples=samples[3],
                                            base_mlp_num_layers=layers, base_mlp_layer_width=width)
    model = cfg.setup(scene_box=None, num_train_data=1)
    with torch.no_grad():
        model.field.field_output_density.net.bias += 1.0
    model.to(dev).train()
    model.field.set_mma_mode(mma)
    model.set_deterministic(deterministic)
    o, d, pa = cpu_ref.synthetic_rays(R, seed=seed)
    rb = pkg.RayBundle(origins=o.to(dev), directions=d.to(dev), pixel_area=pa.to(dev),
                       nears=torch.full((R, 1), 2.0, device=dev), fars=torch.full((R, 1), 6.0, device=dev))
    batch = {"image": torch.rand(R, 3, generator=torch.Generator().manual_seed(seed + 1)).to(dev)}
    return model, rb, batch


def _run_steps(dev, R, layers, width, mma, deterministic, steps, groups=1, ray_chunk=None):
    """-> (gradients after every step, parameters after the last one, reflected rays of the last step)."""
    from reflect_sampling_nerf_amd.parallel import train_step

    model, rb, batch = _train_setup(dev, R, (16, 16, 8, 8), layers, width, mma, deterministic)
    model.weight_grad_groups = groups
    opt = pkg.FusedRAdam(model.get_param_groups()["fields"], lr=1e-3, eps=1e-15)
    torch.manual_seed(5)
    grads = []
    for k in range(steps):
        train_step(model, rb, batch, opt, None, 100 + k, ray_chunk=ray_chunk)
        grads.append({n: p.grad.clone() for n, p in model.field.named_parameters() if p.grad is not None})
    params = {n: p.detach().clone() for n, p in model.field.named_parameters()}
    return grads, params, model._last_num_reflected


def _assert_same_bits(run_a, run_b):
    (ga, pa, _), (gb, pb, _) = run_a, run_b
    for k, (a, b) in enumerate(zip(ga, gb)):
        assert sorted(a) == sorted(b) and a
        for n in a:
            assert torch.equal(a[n], b[n]), f"step {k}: gradient of {n} differs between two deterministic runs"
    for n in pa:
        assert torch.equal(pa[n], pb[n]), f"parameter {n} differs between two deterministic runs"


@pytest.mark.parametrize("mma", ["f32", "bf16x6", "bf16"])
@pytest.mark.parametrize("layers,width,R", [(4, 64, 96), (8, 256, 64)])
def test_deterministic_training_steps_repeat_bitwise(dev, layers, width, R, mma):
    """Two models from one seed, three train_steps with FusedRAdam on the same rays and torch seed, Model.set_deterministic(True):
    every parameter gradient after every step and every parameter at the end are bitwise equal between the runs.  The first step's
    gradients also agree with the default (atomic) mode's within the suite's bound for "same step, other accumulation order"
    (test_weight_grad_groups_two_equals_one: 2e-5 of the tensor's largest entry + 1e-12)."""
    run_a = _run_steps(dev, R, layers, width, mma, True, 3)
    run_b = _run_steps(dev, R, layers, width, mma, True, 3)
    print(f"{layers} x {width} {mma}: {run_a[2]} of {R} rays reflected in the last step")
    _assert_same_bits(run_a, run_b)
    default, _, _ = _run_steps(dev, R, layers, width, mma, False, 1)
    assert sorted(default[0]) == sorted(run_a[0][0])
    for n, g0 in default[0].items():
        assert float((run_a[0][0][n] - g0).abs().max()) <= 2e-5 * float(g0.abs().max()) + 1e-12, n


@pytest.mark.parametrize("setting", [{"groups": 2}, {"ray_chunk": 32}])
def test_deterministic_composes_with_groups_and_ray_chunk(dev, setting):
    """weight_grad_groups = 2 and train_step(ray_chunk=32) change the order of accumulation (other bits than the plain step), but
    for a fixed setting two deterministic runs of two steps repeat bitwise (4 x 64 field, fp32)."""
    run_a = _run_steps(dev, 96, 4, 64, "f32", True, 2, **setting)
    run_b = _run_steps(dev, 96, 4, 64, "f32", True, 2, **setting)
    _assert_same_bits(run_a, run_b)
