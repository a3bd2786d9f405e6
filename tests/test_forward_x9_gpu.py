"""The trunk of the exact-fp32 training forward on the nine-product loop of the 16x16x32 bf16 MFMA shape (rsn_field_kernel.h,
rsn_field_kernel<NB, true, 0 | 4>: the W x W GEMM of every layer l >= 1 through sweep_gemm -- gemm_bf16_s16 over the packed pieces
h_x[l] in the folded instantiation, gemm_f32_x9_s16 with the pieces formed in registers in the unfolded one -- with the row saver
sv_put16, the bias start init_acc16 and the ReLU epilogue store_act16_relu, which writes the slab and the mask words where the fp32
loop's store_act wrote them; the skip layer's accumulators change layout once through the slab).  tests/test_layer_gemms_gpu.py,
test_fold_bottleneck_gpu.py, test_gpu_parity.py and test_multitile_gpu.py judge the forward as they judged the fp32 loop; here is
what the new lane mapping, the 32-lane exchange of the mask nibbles and the new store paths can get wrong at shapes theirs do not
reach.  The index maps themselves are stated in tests/forward_x9_maps.py and held against store_act's in test_forward_x9_cpu.py.

Every comparison is against the fp64 restatement and the per-entry bound K u S of tests/layer_gemm_reference.py (imported), on the
kernel's own input rows, unless stated: the integer cases are bit for bit against the host's integer sums, the folded / unfolded,
multi-job and repeatability cases bit for bit against another launch.  No constant here comes from a run of the kernels.

  1. point halves: 16, 17, 31, 32 and 49 points (the second point half of a wave's tile empty, with one row, lacking one row,
     full, and a second wave that starts in a half), 1, 33 and 300 points; widths 256, 128, 64 and parameter width 200 (padded
     units); nets L2 (one moved GEMM), L3 and L8 with its skip; with and without the analytic normals; both instantiations.
     Every forward record passes the bound and relu_bits[l] equals act[l] > 0 exactly for every trunk layer.
  6. (in the same cases) folded against unfolded: everything upstream of the colour path is bit for bit equal.
  2. integer weights and integer biases, the encoded-input parts zero: layer 0 produces the integer activations relu(b_0) (the
     same at every point of a frustum job: the point maps are item 1's) and every trunk sum is exact in fp32 in any order, so
     act[l] equals the host's integer relu(W_l act[l-1] + b_l) bit for bit and relu_bits[l] equals (that sum > 0).  The live
     units of each layer in turn are confined to one 4-row group of every 32-row block, for each of the eight groups, and one
     unit of that group has a zero row and a zero bias: its pre-activation is exactly 0 and its bit is 0.
  3. no stray stores: saved buffers and outputs poisoned, a device-side count so that the last live wave holds 1, 16, 17 or 31
     rows and whole tiles lie behind it: live rows pass the bound, every row behind the count keeps the poison, relu_bits included.
  4. a launch of two jobs (a level of 45 x 3 points and get_inf_color on 45: the second job starts inside the 128-point tile the
     first ends in, were the tiles shared) equals the two launches of one job bit for bit.
  5. two runs of one case are bit-equal."""
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, ops
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import field_maths_reference as R
from tests import forward_x9_maps as M
from tests import layer_gemm_reference as G
from tests import test_layer_gemms_gpu as LG
from tests import test_normals_seed_gpu as S
from tests.helpers import _POISON, _poisoned
from tests.test_normals_x9_gpu import _integer_field

pytestmark = pytest.mark.gpu

POINTS = {"1": (1, 1), "16": (16, 1), "17": (17, 1), "31": (31, 1), "32": (32, 1), "33": (11, 3), "49": (49, 1), "300": (100, 3)}
WIDTHS = (256, 128, 64, 200)
NETS = ("L2", "L3", "L8")
UPSTREAM = ("sigma", "raw_density", "pred_normals", "n_dot_d", "diff", "tint", "roughness")  # of the colour path


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


def _host(d):
    return {k: v.detach().cpu() for k, v in d.items() if torch.is_tensor(v)}


def _assert_poison(label, key, t):
    if t.numel():
        it, pattern = _POISON[t.dtype]
        assert bool((t.contiguous().view(it) == pattern).all()), f"{label} {key}: rows behind the device-side count were written"


def run_forward(dev, fold, width, net, points, normals, n_live_rays=None, seed=23):
    """One training forward of a frustum level on poisoned buffers -> (failures, level on the host, saved on the host).  Judged: every
    forward record of layer_gemm_reference.restate on the live rows, relu_bits[l] == act[l] > 0 for the trunk layers, and the
    poison in every row behind a device-side count."""
    layers, skips = LG.NETS[net]
    Rn, Sn = points
    f = S._field(width, layers=layers, skips=skips, seed=seed)
    inp = S._rays(Rn, Sn, seed=width + layers + Rn)
    f.to(dev).train()
    f.set_mma_mode("f32")
    lay, ring = LG._kernel(f, "f32", width)
    n_dev = None if n_live_rays is None else torch.tensor([n_live_rays], dtype=torch.int32, device=dev)
    with LG._launching(), LG._poisoned_allocators(f):
        lv = f.evaluate_frustums_train(inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev), inp["eb"].to(dev), n_dev=n_dev,
                                       want_normals=normals, fold=fold)
    n = Rn * Sn
    live = n if n_live_rays is None else n_live_rays * Sn
    label = f"f32{' folded' if fold else ''} w{width} {net} {n} points ({live} live), normals {normals}"
    saved, level = _host(lv["saved"]), _host(lv)
    assert ("bott" in saved) == (not fold) and ("normals" in saved) == normals
    for k, t in saved.items():  # (the normals buffer is allocated by evaluate_frustums_train itself, unpoisoned)
        if k != "normals":
            _assert_poison(label, "saved." + k, t[:, live:] if k in ("act", "relu_bits") else t[live:])
    for k, t in level.items():
        if k != "normals":
            _assert_poison(label, k, t.reshape(n, -1)[live:])
    h = lambda t, *s: t.reshape(n, *s)[:live]  # noqa: E731
    rows = {"enc": h(saved["enc"], -1), "sh": h(saved["sh"], -1), "act": saved["act"].reshape(layers, n, -1)[:, :live],
            "hid": h(saved["hid"], 128), "heads": h(saved["heads"], 8), "raw_density": h(level["raw_density"]),
            "diff": h(level["diff"], 3), "tint": h(level["tint"], 3)}
    if not fold:
        rows["bott"] = h(saved["bott"], -1)
    recs = G.restate(_host(f.state_dict()), lay, rows, layers, skips[0] if skips else -1, "f32", fold, ring)
    assert {f"act[{l}]" for l in range(layers)} | {"hid", "rgb", "head_density", "head_normals"} <= set(recs)
    shares, failures = G.judge(label, "f32", recs, ring)
    print(G.report(label, shares))
    W = saved["act"].shape[2]
    for l in range(layers):
        want = rows["act"][l] > 0
        got = M.decode_relu_bits(saved["relu_bits"][l, :live], W)
        if not torch.equal(got, want):
            p, c = (got != want).nonzero()[0].tolist()
            failures.append(f"[{label}] relu_bits[{l}]: point {p}, unit {c}: bit {int(got[p, c])}, act {float(rows['act'][l][p, c]):.6e}; "
                            f"{int((got != want).sum())} bits differ")
    if normals:
        assert bool(torch.isfinite(level["normals"].reshape(n, 3)[:live]).all()), f"{label}: normals"
    return failures, level, saved


# ---------------------------------------------------------------------------------------------- 1. point halves, 6. folded == unfolded
def _halves_cases():
    c = [(w, "L8", p, True) for w in WIDTHS for p in POINTS]
    c += [(w, n, p, True) for w in (256, 64) for n in ("L2", "L3") for p in ("17", "49")]
    c += [(w, n, "49", False) for w in WIDTHS for n in NETS]
    c += [(256, "L8", p, False) for p in POINTS if p != "49"]
    return c


def _assert_upstream_equal(label, a, b, layers, width, normals):
    """(level, saved) of the unfolded and the folded instantiation: bit for bit upstream of the colour path"""
    (la, sa), (lb, sb) = a, b
    for k in UPSTREAM + (("normals",) if normals else ()):
        assert torch.equal(la[k].view(torch.int32), lb[k].view(torch.int32)), f"{label}: {k} differs between folded and unfolded"
    for k in ("act", "enc", "sh"):
        assert torch.equal(sa[k].view(torch.int32), sb[k].view(torch.int32)), f"{label}: saved.{k} differs between folded and unfolded"
    assert torch.equal(sa["heads"][:, :4].contiguous().view(torch.int32), sb["heads"][:, :4].contiguous().view(torch.int32)), label
    nw = width // 64 if width >= 64 else 1  # mask words a lane half writes per trunk layer
    assert torch.equal(sa["relu_bits"][:layers, :, :, :nw], sb["relu_bits"][:layers, :, :, :nw]), f"{label}: the trunk's ReLU bits differ"


@pytest.mark.parametrize("width,net,points,normals", _halves_cases(),
                         ids=[f"w{w}-{n}-{p}-{'normals' if v else 'plain'}" for w, n, p, v in _halves_cases()])
def test_point_halves(dev, width, net, points, normals):
    res = {}
    for fold in (False, True):
        failures, level, saved = run_forward(dev, fold, width, net, POINTS[points], normals)
        assert not failures, "\n" + "\n".join(failures)
        res[fold] = (level, saved)
    padded = {200: 256}.get(width, width)
    _assert_upstream_equal(f"w{width} {net} {points}", res[False], res[True], LG.NETS[net][0], padded, normals)


# ---------------------------------------------------------------------------------------------- 2. integers
INT_NETS = {"L3": (3, ()), "L4skip": (4, (2,))}
INT_CASES = [(w, n, layer) for w in (64, 256) for n, (L, _) in INT_NETS.items() for layer in range(L)]
N_INT = 49  # a full wave tile and one that ends one row into its second point half


def _integer_net(width, layers, skips, layer, group):
    """_integer_field's trunk x parts (-2 .. 2 on eight rows a column) with every encoded-input part set to zero and every trunk
    bias an integer: layer 0 gives relu(b_0), integers (the same at every point: a frustum's encoded inputs are no integers, and
    the job of explicit means keeps the fp32 loop), and every sum behind it is an integer.  Layer 0's bias is drawn from -12 .. 12.
    The units of `layer` outside 4-row group `group` of every 32-row block get the bias -1e6 (dead), and the group's second unit
    of block 0 a zero row and a zero bias.  -> (field, that unit)"""
    f = _integer_field(width, layers, skips)
    inside = ((torch.arange(width) % 32) // 4) == group
    zero_unit = 4 * group + 1
    g = torch.Generator().manual_seed(width + layers)
    with torch.no_grad():
        for l in range(layers):
            lin = f.mlp_base.layers[l]
            if l == 0 or l in skips:
                lin.weight[:, :99] = 0.0
            lin.bias.copy_(torch.round(lin.bias))
        f.mlp_base.layers[0].bias.copy_(torch.randint(-12, 13, (width,), generator=g).float())
        lin = f.mlp_base.layers[layer]
        lin.bias[~inside] = -1e6
        lin.weight[zero_unit] = 0.0
        lin.bias[zero_unit] = 0.0
    return f, zero_unit


@pytest.mark.parametrize("group", range(8))
@pytest.mark.parametrize("width,net,layer", INT_CASES, ids=[f"w{w}-{n}-layer{l}" for w, n, l in INT_CASES])
def test_integer_sums_row_groups_and_nibbles(dev, width, net, layer, group):
    layers, skips = INT_NETS[net]
    skip = skips[0] if skips else -1
    f, zero_unit = _integer_net(width, layers, skips, layer, group)
    f.to(dev).train()
    f.set_mma_mode("f32")
    inp = S._rays(N_INT, 1, seed=width + layers)
    P = _host(f.state_dict())
    inside = ((torch.arange(width) % 32) // 4) == group
    # the host's integer forward: every sum below 2^24 in magnitude with all its partial sums, in any order
    x, want = None, []
    for l in range(layers):
        w, b = P[f"mlp_base.layers.{l}.weight"].double(), P[f"mlp_base.layers.{l}.bias"].double()
        if l == 0:
            z, s = b.clone(), b.abs()
        else:
            wl = w[:, 99:] if l == skip else w
            z, s = wl @ x + b, wl.abs() @ x.abs() + b.abs()
        assert bool((z == z.round()).all()) and float(s.max()) * 1.01 ** 2 < 2.0 ** 24, "not an exact case"
        want.append(z)
        x = torch.relu(z)
    live = want[layer] > 0
    assert not bool(live[~inside].any())
    frac = float(live[inside].float().mean())
    assert 0.05 < frac < 0.95, f"group {group} of layer {layer}: {frac:.2f} live: not a mixed mask"
    assert float(want[layer][zero_unit]) == 0.0
    for fold in (False, True):
        with LG._launching(), LG._poisoned_allocators(f):
            lv = f.evaluate_frustums_train(inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev), inp["eb"].to(dev), want_normals=True, fold=fold)
        saved = _host(lv["saved"])
        act = saved["act"]
        for l in range(layers):
            z = want[l].expand(N_INT, width)
            assert torch.equal(act[l][:, :width].double(), torch.relu(z)), f"fold {fold}: act[{l}] differs from the host's integer sums"
            assert bool((act[l][:, width:] == 0).all())
            bits = M.decode_relu_bits(saved["relu_bits"][l], act.shape[2])
            assert torch.equal(bits[:, :width], z > 0), f"fold {fold}: relu_bits[{l}] differs from (the host's integer sum > 0)"
            assert not bool(bits[:, width:].any())
        assert not bool(M.decode_relu_bits(saved["relu_bits"][layer], act.shape[2])[:, zero_unit].any()), "the bit of an exact zero is set"


# ---------------------------------------------------------------------------------------------- 3. no stray stores
# (rays in the buffers, live rays), one sample a ray: the last live wave holds 1, 16, 17, 31 rows; 129: one row in a second tile
COUNTS = [(70, 33), (70, 48), (70, 49), (70, 63), (300, 129)]


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])
@pytest.mark.parametrize("cap,live", COUNTS, ids=[f"{c}-{l}" for c, l in COUNTS])
@pytest.mark.parametrize("width", WIDTHS)
def test_no_stray_stores(dev, width, cap, live, fold):
    failures, _, _ = run_forward(dev, fold, width, "L8", (cap, 1), True, n_live_rays=live)
    assert not failures, "\n" + "\n".join(failures)


# ---------------------------------------------------------------------------------------------- 4. multi-job launch
def _launch_jobs(dev, f, fold, which, rays, eb, n_dev, d_inf, sq):
    """rsn_field_forward_train_jobs with the level job, get_inf_color's job, or both (as evaluate_reflect_train builds them), on
    poisoned buffers -> (level, saved, bg, inf_saved) on the host (None for a job that was not launched)"""
    lib = pkg.load_library()
    Rn, Sn = eb.shape[0], eb.shape[1] - 1
    level, saved = _poisoned(f.alloc_train_level(dev, Rn, Sn)), _poisoned(f._alloc_saved(Rn * Sn, dev, fold))
    inf_saved = _poisoned(f._alloc_saved(Rn, dev, fold))
    bg = torch.full((Rn, 3), float("nan"), device=dev)
    fo, fs, fs_inf = ops.field_outputs_struct(level), ops.saved_struct(saved), ops.saved_struct(inf_saved)
    both = (_abi.FieldJob * 2)()
    ops.set_frustum_job(both[0], Rn, n_dev, Sn, *rays, eb)
    both[0].out, both[0].saved = C.pointer(fo), C.pointer(fs)
    both[1].kind, both[1].n_rays, both[1].n_dev, both[1].n_samples = 1, Rn, n_dev.data_ptr(), 1
    both[1].directions, both[1].sqradius, both[1].out_rgb = d_inf.data_ptr(), sq.data_ptr(), bg.data_ptr()
    both[1].saved = C.pointer(fs_inf)
    jobs = (_abi.FieldJob * 2)()
    picked = {"both": (0, 1), "level": (0,), "inf": (1,)}[which]
    for k, j in enumerate(picked):
        C.memmove(C.byref(jobs[k]), C.byref(both[j]), C.sizeof(_abi.FieldJob))
    desc, pk = f.field_desc(fold), f.packed_weights(fold)
    with LG._launching():
        check(lib.rsn_field_forward_train_jobs(C.byref(desc), ptr(pk), len(picked), jobs, ops._stream()))
    return _host(level), _host(saved), bg.cpu(), _host(inf_saved)


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "plain"])
@pytest.mark.parametrize("width", [256, 64])
def test_jobs_launch_equals_separate_launches(dev, width, fold):
    layers, skips = LG.NETS["L8"]
    Mr, Sn = 45, 3
    f = S._field(width, layers=layers, skips=skips, seed=31)
    f.to(dev).train()
    f.set_mma_mode("f32")
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    sq, d_inf = inf["sq"][:Mr].contiguous().to(dev), inf["d"][:Mr].contiguous().to(dev)
    n_dev = torch.tensor([Mr], dtype=torch.int32, device=dev)
    inp = S._rays(Mr, Sn, seed=width + Sn)
    rays, eb = (inp["o"].to(dev), d_inf, inp["pa"].to(dev)), inp["eb"].to(dev)
    lv2, sv2, bg2, is2 = _launch_jobs(dev, f, fold, "both", rays, eb, n_dev, d_inf, sq)
    lv1, sv1, _, _ = _launch_jobs(dev, f, fold, "level", rays, eb, n_dev, d_inf, sq)
    _, _, bg1, is1 = _launch_jobs(dev, f, fold, "inf", rays, eb, n_dev, d_inf, sq)
    assert bool(torch.isfinite(sv2["act"]).all()) and bool(torch.isfinite(is2["act"]).all()) and bool(torch.isfinite(bg2).all())
    for name, a, b in (("level", lv2, lv1), ("saved", sv2, sv1), ("inf saved", is2, is1), ("inf rgb", {"bg": bg2}, {"bg": bg1})):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{name} {k}: the jobs launch differs from the single launch"


# ---------------------------------------------------------------------------------------------- 5. repeatability
@pytest.mark.parametrize("width,net,points", [(256, "L8", "300"), (64, "L3", "49")])
def test_two_runs_are_bit_equal(dev, width, net, points):
    (fa, la, sa), (fb, lb, sb) = (run_forward(dev, True, width, net, POINTS[points], True) for _ in range(2))
    assert not fa and not fb
    for a, b in ((la, lb), (sa, sb)):
        for key in a:
            assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), f"{key} differs between two runs"
