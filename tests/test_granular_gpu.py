"""The granular field evaluation -- explicit Gaussians (RSN_MODE_GAUSS) and a caller-supplied embedding (RSN_MODE_EMB) -- and the
standalone geometry kernels against fp64 (tests/granular_reference.py), through the C ABI, so that every pointer combination is
reachable: all four MMA modes, sizes at which every workgroup walks its persistent loop at least twice and the last tile is ragged,
333 points (three tiles, the last with a partly valid and a skipped wave), cov_diag / view_dirs / roughness / output pointers NULL,
the padded units of a 200-wide field, the training variant on both exact-fp32 descriptors, and the Python wrappers' bits.  Mesh,
texture and point-cloud export push all their points through these two modes.

Every output buffer is poisoned and 64 rows longer than N: the rows behind N must keep the poison.  Once a launch of this file has
raised, no later test starts another one.

Bounds.  None is measured on the code under test.
  f32, bf16x6 against fp64: TOL = 1e-4 on color, diff, tint, roughness; TOL x (1 + |ref|) on sigma, raw_density, raw_roughness and
    the embedding; TOL_UNIT = 5e-4 on pred_normals and n_dot_d (test_gpu_parity's constants).
  bf16x3: 2e-3 in TOL's place and 10 x TOL_UNIT (test_field_level_split_bf16_modes' rule).
  bf16: TOL_BF16 = 3e-2 in TOL's place; pred_normals and n_dot_d per point within 4 x the error of the rounded-bf16 fp64 forward
    (granular_reference.rounded) at the worst point of the kernel's tile, plus 2^-8: field_maths_reference's FACTOR = 4 rule with
    the rounded reference in the float32 oracle's place.
  cov_diag == NULL (undamped IPE: the phase fl32(fl32(2 pi x) f) of the top frequencies is off by up to ~5e-2 rad, which is fp32's
    and shared by the float32 oracle): per output, 4 x worst |cpu_ref in float32 - fp64| + one fp32 ulp of the output's scale
    (field_maths_reference.compare).  In plain bf16 that figure is an allowance on top of the bf16 bounds: the error there is the
    GEMMs' rounding plus the same fp32 phases.  That rule is blind below the phase error (~1e-3), so the same outputs are also held
    to the mode's ordinary bounds against the float32 ORACLE, whose phases the kernels reproduce.
  Training normals: NORMALS_MEAN / NORMALS_Q99 of test_multitile_gpu on the mean and the 0.99 quantile.
  Geometry kernels: the `compare` rule per input class against the float32 cpu_ref.gaussian_blob / cpu_ref.contract, and a float32
    torch restatement of the reflection.
  pred_normals / n_dot_d leave out the points whose fp64 |raw normal head| is below 1e-2, the training normals those whose fp64
    |d raw_density / d mean| is below 1e-3 of the median; at most 0.5 % of a case (tests/test_granular_cpu.py checks the cap on the
    reference alone).
  Bit-equalities: torch.equal on the integer view.

Measured on MI355X: see MEASURED below and DESIGN.md section 4.14.1."""
import contextlib
import copy
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, mesh, ops
from reflect_sampling_nerf_amd._abi import check, ptr
from tests import field_maths_reference as FM
from tests import granular_reference as G
from tests.helpers import _POISON, _poisoned, default_dtype, locate, multitile_geometry

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
TOL = G.TOL  # the bounds of the docstring live beside the rule, in granular_reference
NORMALS_MEAN, NORMALS_Q99 = 3.5e-2, 6.5e-1  # test_multitile_gpu
EQUIV = 2e-6      # test_fold_bottleneck_gpu.EQUIV: the colour path of the folded descriptor against the two-GEMM one
TAIL = 64
MODES = ["f32", "bf16x6", "bf16x3", "bf16"]
# MEASURED on MI355X (256 CUs), worst over the cases of this file, as value (bound); also DESIGN.md section 4.14.1:
#   f32 / bf16x6 (Gaussians, embedding, training; looping and 333 points): color 4.4e-7, diff 3.7e-7, tint 2.8e-7, roughness 2.1e-7
#     (1e-4); sigma 5.6e-7, raw_density 9.1e-7, raw_roughness 8.9e-7, embedding 3.7e-6, each / (1 + |ref|) (1e-4); pred_normals
#     1.6e-5, n_dot_d 1.5e-5 (5e-4).  The loop's iterations >= 1 show the figures of iteration 0.
#   bf16x3: color 4.4e-7, sigma 5.2e-7, raw_roughness 1.0e-6, embedding 3.6e-6 (2e-3); pred_normals 1.4e-5, n_dot_d 1.4e-5 (5e-3).
#   bf16: color 1.2e-4, diff 8.0e-5, tint 8.3e-5, roughness 6.0e-5, sigma 7.9e-5, raw_density 1.4e-4, raw_roughness 2.3e-4,
#     embedding 6.1e-4 (3e-2); pred_normals 2.5e-3 and n_dot_d 2.5e-3 = 0.21 / 0.25 of 4 x the tile-worst rounded-bf16 error + 2^-8.
#     The rounded-bf16 forward's own worst error is 2.5e-3 / 2.8e-3: kernel / rounded = 1.00 / 0.91, the kernels' error IS the
#     operand rounding, so FACTOR = 4 is not used up and needed no second look.
#   cov_diag == NULL, f32, kernel / float32 oracle / bound: color 8.2e-5 / 8.2e-5 / 3.3e-4, sigma 2.7e-4 / 2.7e-4 / 1.1e-3,
#     embedding 1.0e-3 / 1.0e-3 / 4.1e-3, pred_normals 2.6e-3 / 2.6e-3 / 1.0e-2; against the float32 oracle itself: color 1.2e-7,
#     sigma 3.9e-7, embedding 8.1e-8 (1e-4), pred_normals 6.6e-7 (5e-4).  bf16: every error below its allowance alone (embedding
#     1.1e-3 of 3.4e-3, tint 1.2e-4 of 2.0e-4); against the float32 oracle color 1.1e-4, embedding 7.1e-4 (3e-2), unit vectors 0.20.
#   training normals: mean 3.3e-4 (3.5e-2), 0.99-quantile 1.4e-3 (6.5e-1), both descriptors, bit-equal; colour folded against
#     two-GEMM 1.5e-7 of its largest value (2e-6).  No point of any case fell under an exclusion floor.
#   geometry, kernel / float32 oracle / bound of the class with the largest share: rsn_gaussians mean 0.23 of its bound (area_1e-6),
#     cov 0.20 (axis_x; largest values 6.1e-3 / 1.2e-2 / 5.4e-2 in far_1e3); rsn_contract mean 2.1e-7 / 2.7e-7 / 1.3e-6, cov 5.6e-8 /
#     5.6e-8 / 3.4e-7; rsn_reflection 1.1e-7 / 1.1e-7 / 5.7e-7, n_dot_d 1.3e-7 / 1.3e-7 / 7.5e-7.

SHAPES, ALL, UNIT = G.SHAPES, G.ALL, G.UNIT


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


_dead, _dev_fields, _inputs, _refs = [], {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_caches():
    """The fields, inputs and references the tests of this file share are dropped when its last test has run."""
    yield
    for cache in (_dev_fields, _inputs, _refs):
        cache.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _launching():
    """GPU work of this file: once a launch has raised, no later test starts another one on the device."""
    if _dead:
        pytest.fail(f"an earlier launch of this file failed ({_dead[0]}): not launching again")
    try:
        yield
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        _dead.append(repr(e))
        raise


def _field(dev, key, mode="f32"):
    if key not in _dev_fields:
        f, P, fs = G.make_field(*key)
        _dev_fields[key] = (copy.deepcopy(f).to(dev).eval(), P, fs)
    f, P, fs = _dev_fields[key]
    f.set_mma_mode(mode)
    return f, P, fs


def _input_set(dev, label, cus):
    """One input set of granular_reference.input_sets, on the host and on the device."""
    if label not in _inputs:
        (_, key, kind, N, seed), = [s for s in G.input_sets(cus) if s[0] == label]
        host = G.build_inputs(key, kind, N, seed)
        _inputs[label] = (key, N, host, {k: (None if v is None else v.to(dev)) for k, v in host.items()})
    return _inputs[label]


def _cached(name, fn):
    if name not in _refs:
        _refs[name] = fn()
    return _refs[name]


def _first(d, n):
    return {k: v[:n] for k, v in d.items()}


def _geometry(label, mode, width, kind, N, cus, loop, layers=8):
    """(tile, grid) of the launch that serves (mode, kernel width, kind); loop: asserted with helpers.multitile_geometry.
    layers: the ring serves trunks of up to 10 layers (RSN_RING_MAX_LAYERS, rsn_launch_field_bf16)."""
    if mode == "bf16":
        tile, units = (256, cus) if (kind == "gauss" and width == 256 and layers <= 10) else (128, 2 * cus)  # the ring / rsn_field_bf16_kernel<NB>
    else:
        tile, units = 128, cus
    if loop:
        _, grid, _ = multitile_geometry(label, [N], tile, units, min_per_wg=2)
    else:
        grid = min(-(-N // tile), units)
    return tile, grid


# ---------------------------------------------------------------------------------------------- launches
def _alloc(dev, N, names, emb_w=0):
    bufs = {k: torch.empty((N + TAIL,) + SHAPES[k], device=dev, dtype=f32) for k in names}
    if emb_w:
        bufs["embedding"] = torch.empty(N + TAIL, emb_w, device=dev, dtype=f32)
    return _poisoned(bufs)


def _host(label, bufs, N):
    """The live rows on the host, after checking that the 64 rows behind them kept the poison and that no live row did."""
    out = {}
    for k, t in bufs.items():
        it, pattern = _POISON[t.dtype]
        w = t.view(it)
        assert bool((w[N:] == pattern).all()), f"{label} {k}: rows behind n_points were written"
        assert not bool((w[:N] == pattern).any()), f"{label} {k}: live rows left unwritten"
        out[k] = t[:N].cpu()
    return out


def _gauss(label, f, N, inp, names=ALL, emb=True, cov=True, dirs=True):
    lib = _abi.load_library()
    dev = inp["means"].device
    outs = _alloc(dev, N, names, f.width if emb else 0)
    fo = ops.field_outputs_struct(outs)
    desc, pk = f.field_desc(), f.packed_weights()
    with _launching():
        check(lib.rsn_field_forward_gaussians(C.byref(desc), ptr(pk), N, ptr(inp["means"]), ptr(inp["cov_diag"] if cov else None),
                                              ptr(inp["view_dirs"] if dirs else None), C.byref(fo), ptr(outs.get("embedding")),
                                              ops._stream()))
    return _host(label, outs, N)


def _emb(label, f, N, inp, names=ALL, dirs=True, rough=True):
    lib = _abi.load_library()
    outs = _alloc(inp["embedding"].device, N, names)
    fo = ops.field_outputs_struct(outs)
    desc, pk = f.field_desc(), f.packed_weights()
    with _launching():
        check(lib.rsn_field_forward_embedding(C.byref(desc), ptr(pk), N, ptr(inp["embedding"]), ptr(inp["view_dirs"] if dirs else None),
                                              ptr(inp["roughness"] if rough else None), C.byref(fo), ops._stream()))
    return _host(label, outs, N)


def _equal_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------- 1. Gaussians, eval, looping
def _loop_n(mode, cus):
    return G.n_loop256(cus) if mode == "bf16" else G.n_loop128(cus)


@pytest.mark.parametrize("mode", MODES)
def test_gaussians_eval_loop_against_fp64(dev, cus, mode):
    """rsn_field_forward_gaussians at width 256, damped, with directions and the embedding output: every output of every point."""
    key, _, host, on_dev = _input_set(dev, "loop gauss", cus)
    f, P, fs = _field(dev, key, mode)
    N = _loop_n(mode, cus)
    label = f"gauss loop {mode}"
    tile, grid = _geometry(label, mode, 256, "gauss", N, cus, True)
    ref = _cached("loop gauss", lambda: G.gauss_reference(P, fs, host["means"], host["cov_diag"], host["view_dirs"]))
    r16 = _cached("loop gauss r16", lambda: G.rounded(G.gauss_reference, torch.bfloat16)(
        P, fs, host["means"], host["cov_diag"], host["view_dirs"])) if mode == "bf16" else None
    got = _gauss(label, f, N, _first(on_dev, N))
    G.judge(label, mode, got, _first(ref, N), N, tile, grid, None if r16 is None else _first(r16, N))


# ---------------------------------------------------------------------------------------------- 2. embedding, eval, looping
# (a) the get_pred_normals / get_diff / get_tint / get_roughness call; (b) get_mid; (c) directions without an explicit roughness
# (reachable only through the ABI): rho from the roughness head, n_dot_d from the directions
FLAVOURS = {"heads": dict(names=ALL, dirs=False, rough=False), "mid": dict(names=("color",), dirs=True, rough=True),
            "dirs_head_rho": dict(names=ALL, dirs=True, rough=False)}


def _emb_refs(name, P, fs, host, flavour, bf16):
    fl = FLAVOURS[flavour]
    args = (P, fs, host["embedding"], host["view_dirs"] if fl["dirs"] else None, host["roughness"] if fl["rough"] else None,
            len(fl["names"]) > 1)
    ref = _cached(f"{name} {flavour}", lambda: G.emb_reference(*args))
    r16 = _cached(f"{name} {flavour} r16", lambda: G.rounded(G.emb_reference, torch.bfloat16)(*args)) if bf16 else None
    return ref, r16


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("mode", MODES)
def test_embedding_eval_loop_against_fp64(dev, cus, mode, flavour):
    """rsn_field_forward_embedding at width 256; in plain bf16 this is rsn_field_bf16_kernel<8>, which only this mode reaches."""
    key, _, host, on_dev = _input_set(dev, "loop emb", cus)
    f, P, fs = _field(dev, key, mode)
    N = _loop_n(mode, cus)
    label = f"emb loop {mode} {flavour}"
    tile, grid = _geometry(label, mode, 256, "emb", N, cus, True)
    ref, r16 = _emb_refs("loop emb", P, fs, host, flavour, mode == "bf16")
    fl = FLAVOURS[flavour]
    got = _emb(label, f, N, _first(on_dev, N), **fl)
    if not fl["dirs"]:
        assert float(got["n_dot_d"].abs().max()) == 0.0
    G.judge(label, mode, got, _first(ref, N), N, tile, grid, None if r16 is None else _first(r16, N))


# ---------------------------------------------------------------------------------------------- 3. small and ragged
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("key", G.SMALL_FIELDS, ids=[f"{l}x{w}" for l, w in G.SMALL_FIELDS])
def test_small_ragged_all_widths(dev, cus, key, mode):
    """333 points at (8, 64), (4, 128), (8, 256) and (8, parameter width 200): Gaussians with cov_diag == NULL, Gaussians without
    directions, the embedding's head getters and get_low (colour only, no directions)."""
    N, k = G.N_SMALL, G.SMALL_FIELDS.index(key)
    f, P, fs = _field(dev, key, mode)
    W, bf16 = f.width, mode == "bf16"
    rnd = (lambda fn: G.rounded(fn, torch.bfloat16)) if bf16 else (lambda fn: (lambda *a: None))  # noqa: E731
    # ---- Gaussians, cov_diag == NULL
    label = f"small gauss undamped {key} {mode}"
    _, _, host, on_dev = _input_set(dev, f"small gauss undamped {key}", cus)
    assert host["cov_diag"] is None
    tile, grid = _geometry(label, mode, W, "gauss", N, cus, False)
    args = (P, fs, host["means"], None, host["view_dirs"])
    ref, ora = G.gauss_reference(*args), G.gauss_reference(*args, dtype=f32)
    got = _gauss(label, f, N, on_dev, cov=False)
    r16 = rnd(G.gauss_reference)(*args)
    if bf16:
        G.judge(label, mode, got, ref, N, tile, grid, r16, allow=G.oracle_allowance(ref, ora, N))
        r16 = {k: ora[k].double() + (r16[k] - ref[k]) for k in UNIT}  # the GEMMs' rounding noise, centred on the float32 oracle
    else:
        assert bool((got["embedding"][:, fs.width:] == 0).all())
        G.judge_against_oracle(label, got, ref, ora, N)
    # The kernels form the float32 oracle's phases fl32(fl32(2 pi x) f) in its order, so against the ORACLE the undamped phase
    # error drops out and the mode's ordinary bounds hold: what the rule above cannot see below ~1e-3 is seen here.
    G.judge(label + ", against the float32 oracle", mode, got, ora, N, tile, grid, r16)
    # ---- Gaussians, view_dirs == NULL
    label = f"small gauss no dirs {key} {mode}"
    _, _, host, on_dev = _input_set(dev, f"small gauss {key}", cus)
    args = (P, fs, host["means"], host["cov_diag"], None)
    got = _gauss(label, f, N, on_dev, dirs=False)
    assert float(got["n_dot_d"].abs().max()) == 0.0
    G.judge(label, mode, got, G.gauss_reference(*args), N, tile, grid, rnd(G.gauss_reference)(*args) if bf16 else None)
    # ---- embedding: the head getters, get_low
    _, _, host, on_dev = _input_set(dev, f"small emb {key}", cus)
    assert host["embedding"].shape == (N, W) and bool((host["embedding"][:, fs.width:] == 0).all())
    tile, grid = _geometry(label, mode, W, "emb", N, cus, False)
    for flavour, want_all in (("heads", True), ("low", False)):
        label = f"small emb {flavour} {key} {mode}"
        args = (P, fs, host["embedding"], None, None, want_all)
        got = _emb(label, f, N, on_dev, names=ALL if want_all else ("color",), dirs=False, rough=False)
        G.judge(label, mode, got, G.emb_reference(*args), N, tile, grid, rnd(G.emb_reference)(*args) if bf16 else None)
    if fs.width != W:  # Field._heads pads a 200-wide embedding with the zeros the direct call was given
        low = f.get_low(on_dev["embedding"][:, :fs.width])
        torch.cuda.synchronize()
        assert low.shape == (N, 3) and _equal_bits(low.cpu(), got["color"])


# ---------------------------------------------------------------------------------------------- 4. NULL outputs
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_null_output_pointers(dev, cus, mode):
    """Gaussians with only `sigma` set, the embedding with only `color` set: the bits of the call with the other outputs, nothing
    else passed (no decoys), the rows behind N untouched.  The embedding's colour is the mid colour when neither diff nor tint is
    asked for, so its partner is the call with every output BUT those two."""
    N, key = G.N_SMALL, (8, 256)
    f, _, _ = _field(dev, key, mode)
    _, _, _, g_dev = _input_set(dev, f"small gauss {key}", cus)
    full = _gauss(f"null outputs gauss all {mode}", f, N, g_dev)
    only = _gauss(f"null outputs gauss sigma {mode}", f, N, g_dev, names=("sigma",), emb=False)
    assert list(only) == ["sigma"] and _equal_bits(only["sigma"], full["sigma"])
    _, _, _, e_dev = _input_set(dev, f"small emb {key}", cus)
    others = tuple(k for k in ALL if k not in ("diff", "tint"))
    full = _emb(f"null outputs emb all but diff, tint {mode}", f, N, e_dev, names=others)
    only = _emb(f"null outputs emb color {mode}", f, N, e_dev, names=("color",))
    assert list(only) == ["color"] and _equal_bits(only["color"], full["color"])
    both = _emb(f"null outputs emb all {mode}", f, N, e_dev)  # with diff and tint the colour is diff + tint * mid
    assert not _equal_bits(both["color"], full["color"])
    assert float((both["color"].double() - (both["diff"].double() + both["tint"].double() * full["color"].double())).abs().max()) <= 2.0 ** -22
    for k in others:
        if k != "color":
            assert _equal_bits(both[k], full[k]), k


# ---------------------------------------------------------------------------------------------- 5. Gaussians, training
def test_gaussians_training_loop_both_descriptors(dev, cus):
    """rsn_field_forward_gaussians_train at width 256 on RSN_MMA_F32 and on the folded descriptor: outputs against fp64, the two
    descriptors against each other under test_fold_bottleneck_gpu's rule (everything upstream of the colour path bit for bit, the
    colour within 2e-6 of its largest value), saved.normals against fp64 autograd."""
    lib = _abi.load_library()
    key, N, host, on_dev = _input_set(dev, "train gauss", cus)
    assert N == G.n_loop128(cus)
    f, P, fs = _field(dev, key, "f32")
    tile, grid = _geometry("gauss train", "f32", 256, "gauss", N, cus, True)
    ref = G.gauss_reference(P, fs, host["means"], host["cov_diag"], host["view_dirs"])
    nref, gn = G.gauss_normals_reference(P, fs, host["means"], host["cov_diag"])
    keep_n = G.kept_points("gauss train normals", gn, G.GRAD_MIN_REL * float(gn.median()))
    res = {}
    for fold in (False, True):
        label = f"gauss train {'folded' if fold else 'f32'}"
        outs = _alloc(dev, N, ALL, f.width)
        saved = _poisoned(f.alloc_saved_folded(N, dev) if fold else f.alloc_saved(N, dev))
        normals = _poisoned({"normals": torch.empty(N + TAIL, 3, device=dev, dtype=f32)})
        saved["normals"] = normals["normals"]
        fo, fsv = ops.field_outputs_struct(outs), ops.saved_struct(saved)
        desc, pk = f.field_desc(fold), f.packed_weights(fold)
        assert int(desc.mma_mode) == (_abi.RSN_MMA_F32_FOLDED if fold else _abi.RSN_MMA_F32) and ("bott" in saved) == (not fold)
        with _launching():
            check(lib.rsn_field_forward_gaussians_train(C.byref(desc), ptr(pk), N, ptr(on_dev["means"]), ptr(on_dev["cov_diag"]),
                                                        ptr(on_dev["view_dirs"]), C.byref(fo), ptr(outs["embedding"]), C.byref(fsv),
                                                        ops._stream()))
        got = _host(label, outs, N)
        got["normals"] = _host(label, normals, N)["normals"]
        for k in ("enc", "act", "sh", "hid", "relu_bits") + (() if fold else ("bott",)):  # every saved row was written
            it, pattern = _POISON[saved[k].dtype]
            w = saved[k].view(it) == pattern
            if k == "relu_bits":  # [L+1, N, 2, 4] words; mlp_mid's 128 units (layer L) fill two of a lane half's four
                w = torch.cat([w[:-1].reshape(-1, 8), w[-1][:, :, :2].reshape(-1, 4).repeat(1, 2)])
            left = int(w.all(dim=-1).sum())
            assert left == 0, f"{label} saved.{k}: {left} rows left unwritten"
        assert _equal_bits(saved["act"][-1].cpu(), got["embedding"]), f"{label}: saved.act[L-1] is not the embedding output"
        heads = saved["heads"].cpu().double()
        assert float((heads[:, :3] - ref["normal_head"]).abs().max()) <= TOL and float((heads[:, 3] - ref["raw_roughness"]).abs().max()) <= TOL
        del saved, outs
        G.judge(label, "f32", {k: v for k, v in got.items() if k != "normals"}, ref, N, tile, grid)
        e = (got["normals"].double() - nref).abs().amax(1)
        ek = e[keep_n]
        w, i, t, it_, _, _ = locate(e * keep_n.double(), tile, grid)
        print(f"[{label}] normals: mean {float(ek.mean()):.3e} (bound {NORMALS_MEAN:.1e}), 0.99-quantile {float(ek.quantile(0.99)):.3e} "
              f"(bound {NORMALS_Q99:.1e}); worst {w:.3e} at point {i}, tile {t}, iteration {it_}; {int((~keep_n).sum())} points left out")
        assert float(ek.mean()) <= NORMALS_MEAN and float(ek.quantile(0.99)) <= NORMALS_Q99
        assert float((got["normals"].double().norm(dim=-1) - 1).abs().max()) <= 1e-5
        res[fold] = got
    a, b = res[False], res[True]
    for k in a:
        if k != "color":
            assert _equal_bits(a[k], b[k]), f"folded against two-GEMM: {k} differs"
    err, top = float((a["color"].double() - b["color"].double()).abs().max()), float(a["color"].abs().max())
    print(f"[gauss train] colour, folded against two-GEMM: {err / top:.3e} of the largest value (bound {EQUIV:.0e})")
    assert err <= EQUIV * top


# ---------------------------------------------------------------------------------------------- 6. wrappers
def test_wrappers_return_the_bits_of_the_direct_calls(dev, cus):
    """Field.evaluate_gaussians, get_density and _heads at a looping size against the ABI calls; a mesh.density_grid in three
    uneven chunks against one whole-grid call."""
    N = G.n_loop128(cus)
    key, _, _, g_dev = _input_set(dev, "loop gauss", cus)
    f, _, _ = _field(dev, key, "f32")
    g_dev = _first(g_dev, N)
    direct = _gauss("wrappers gauss", f, N, g_dev, names=ALL)
    with _launching():
        lv = f.evaluate_gaussians(g_dev["means"], g_dev["cov_diag"], g_dev["view_dirs"], want_embedding=True)
        sig, emb = f.get_density(g_dev["means"], torch.diag_embed(g_dev["cov_diag"]))
    for k, v in lv.items():
        assert _equal_bits(v.cpu().reshape(direct[k].shape), direct[k]), f"evaluate_gaussians {k}"
    assert sig.shape == (N, 1) and _equal_bits(sig.cpu().reshape(N), direct["sigma"]) and _equal_bits(emb.cpu(), direct["embedding"])
    _, _, _, e_dev = _input_set(dev, "loop emb", cus)
    e_dev = _first(e_dev, N)
    direct = _emb("wrappers emb heads", f, N, e_dev, dirs=False, rough=False)
    mid = _emb("wrappers emb mid", f, N, e_dev, names=("color",))
    with _launching():
        hd = f._heads(e_dev["embedding"])
        gm = f.get_mid(e_dev["view_dirs"], e_dev["roughness"].reshape(N, 1), e_dev["embedding"])
    for k in ("color", "pred_normals", "diff", "tint", "roughness", "raw_density", "sigma", "raw_roughness"):
        assert _equal_bits(hd[k].cpu().reshape(direct[k].shape), direct[k]), f"_heads {k}"
    assert _equal_bits(gm.cpu(), mid["color"])
    # a chunked density grid: about N voxels, neither the grid nor a chunk a multiple of the tile
    nx, ny = 41, 43
    nz = N // (nx * ny)
    n = nx * ny * nz
    multitile_geometry("density_grid, whole", [n], 128, cus, min_per_wg=2)
    chunk = n * 3 // 7
    assert chunk % 128 and (n - 2 * chunk) % 128 and 0 < n - 2 * chunk < chunk
    with _launching():
        whole = mesh.density_grid(f, mesh.DEFAULT_BOUNDS, (nx, ny, nz), chunk=n)
        parts = mesh.density_grid(f, mesh.DEFAULT_BOUNDS, (nx, ny, nz), chunk=chunk)
    assert whole.shape == (nz, ny, nx) and bool(torch.isfinite(whole).all()) and float(whole.std()) > 0
    assert _equal_bits(whole.cpu(), parts.cpu())


# ---------------------------------------------------------------------------------------------- 7. geometry kernels
def _check(v):
    print(v.report())
    assert v.ok, "\n" + v.report()


def test_gaussians_and_contract_kernels_against_fp64(dev):
    """rsn_gaussians -> rsn_contract on field_maths_reference.build_inputs(): 2,680 samples (11 workgroups, the last one partial),
    per input class against fp64; rsn_contract on the bits rsn_gaussians wrote."""
    lib = _abi.load_library()
    inp, S = FM.build_inputs(), FM.S
    cls, names = FM.point_class(inp), inp["names"]
    n = cls.numel()
    assert n > 256 and n % 256
    per = lambda t: t.repeat_interleave(S, 0).contiguous().to(dev)  # noqa: E731
    o, d, pa = per(inp["o"]), per(inp["d"]), per(inp["pa"])
    t0, t1 = inp["eb"][:, :-1].reshape(-1).contiguous().to(dev), inp["eb"][:, 1:].reshape(-1).contiguous().to(dev)
    out = _poisoned({"mean": torch.empty(n + TAIL, 3, device=dev), "cov": torch.empty(n + TAIL, 9, device=dev)})
    with _launching():
        check(lib.rsn_gaussians(n, ptr(o), ptr(d), ptr(pa), ptr(t0), ptr(t1), ptr(out["mean"]), ptr(out["cov"]), ops._stream()))
    got = _host("rsn_gaussians", out, n)

    def blob(dt):
        with default_dtype(dt):
            eb = inp["eb"].to(dt)
            m, c = cpu_ref.gaussian_blob(inp["o"].to(dt), inp["d"].to(dt), inp["pa"].to(dt).reshape(-1, 1), eb[:, :-1], eb[:, 1:])
            return m.reshape(n, 3), c.reshape(n, 9)

    (m64, c64), (m32, c32) = blob(f64), blob(f32)
    _check(FM.compare("rsn_gaussians", "mean", got["mean"], m64, m32, cls, names))
    _check(FM.compare("rsn_gaussians", "cov", got["cov"], c64, c32, cls, names))
    # the contraction of what the kernel above wrote
    mk, ck = got["mean"].contiguous(), got["cov"].contiguous()
    assert bool((mk.norm(dim=-1) > 1).any()) and bool((mk.norm(dim=-1) < 1).any())
    out = _poisoned({"mean": torch.empty(n + TAIL, 3, device=dev), "cov": torch.empty(n + TAIL, 9, device=dev)})
    mk_d, ck_d = mk.to(dev), ck.to(dev)
    with _launching():
        check(lib.rsn_contract(n, ptr(mk_d), ptr(ck_d), ptr(out["mean"]), ptr(out["cov"]), ops._stream()))
    got = _host("rsn_contract", out, n)
    m64, c64 = G.contract(mk, ck.reshape(n, 3, 3))
    with default_dtype(f32):
        m32, c32 = cpu_ref.contract(mk, ck.reshape(n, 3, 3))
    _check(FM.compare("rsn_contract", "mean", got["mean"], m64, m32, cls, names))
    _check(FM.compare("rsn_contract", "cov", got["cov"], c64.reshape(n, 9), c32.reshape(n, 9), cls, names))
    assert float(got["cov"][:, [0, 4, 8]].min()) >= 0.0


def test_reflection_kernel_against_fp64(dev):
    """rsn_reflection on unit normals, n = d, n = -d, n perpendicular to d, a zero normal and directions of length 0.5 and 2, with
    both outputs, with refl == NULL and with ndd == NULL."""
    lib = _abi.load_library()
    ri = G.reflection_inputs()
    n = ri["d"].shape[0]
    assert n > 256 and n % 256
    d, nrm = ri["d"].to(dev), ri["n"].to(dev)
    runs = {}
    for which in (("refl", "ndd"), ("ndd",), ("refl",)):
        out = _poisoned({k: torch.empty((n + TAIL, 3) if k == "refl" else (n + TAIL,), device=dev) for k in which})
        with _launching():
            check(lib.rsn_reflection(n, ptr(d), ptr(nrm), ptr(out.get("refl")), ptr(out.get("ndd")), ops._stream()))
        runs[which] = _host("rsn_reflection " + "+".join(which), out, n)
    both = runs[("refl", "ndd")]
    assert _equal_bits(runs[("ndd",)]["ndd"], both["ndd"]) and _equal_bits(runs[("refl",)]["refl"], both["refl"])
    (r64, d64), (r32, d32) = G.reflection(ri["d"], ri["n"]), G.reflection(ri["d"], ri["n"], dtype=f32)
    _check(FM.compare("rsn_reflection", "reflection", both["refl"], r64, r32, ri["cls"], ri["names"]))
    _check(FM.compare("rsn_reflection", "n_dot_d", both["ndd"], d64, d32, ri["cls"], ri["names"]))
