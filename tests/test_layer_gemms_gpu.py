"""Every GEMM of the three training kernel families against fp64, layer by layer (tests/layer_gemm_reference.py): the forward
chain -- trunk layers with the skip concatenation, the heads, bottleneck -> mlp_mid -> RGB, folded and unfolded -- and the
transposed chain of the dX sweep, each GEMM restated on the input row the kernel itself saved and compared with the output row it
wrote, entry by entry, every point and every column, nothing left out.  A failing assertion names family, record, layer, point,
column, |err|, B and S; every test prints the worst |err| / B per record.

One launch pair per case: evaluate_frustums_train(want_normals=True, fold=...) then train_graph._field_backward(need_input=True,
fold=...) with random normal upstream gradients on sigma, colour, pred_normals, n_dot_d and roughness, all buffers poisoned first.
The get_inf_color job and a frustum level with a device-side count go through evaluate_reflect_train and
train_graph._reflect_field_backward.  Which kernel served a case is asserted through train_layout() (enc_cols == 128: the LDS-ring
kernels; narrow_dtype bf16: the plain ring).

Bounds: layer_gemm_reference.bound (K u S, + C_X6 S for bf16x6, + half a bf16 ulp for the rows the plain-bf16 kernels store as
bf16), derived there; d_input by field_maths_reference.compare against the float32 restatement.  Nothing is measured on the kernels.
The recorded shares of the bound: profiles/layer_gemms.json (tools/layer_gemms_report.py), DESIGN 4.20.

Shapes: the library refuses none of them (rsn_last_error); none is left out."""
import contextlib

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import train_graph
from tests import field_maths_reference as R
from tests import layer_gemm_reference as G
from tests import test_normals_seed_gpu as S
from tests.helpers import _POISON, _poisoned

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
NETS = {"L2": (2, ()), "L3": (3, ()), "L4": (4, (2,)), "L6": (6, (4,)), "L8": (8, (4,))}
POINTS = {"1": (1, 1), "33": (11, 3), "300": (100, 3)}  # 300: a ragged last tile of both tilings, a second wave starting mid-tile
ALL_POINTS = ("1", "33", "300")


def _cases():
    c = []
    for fold in (False, True):  # exact fp32, per wave
        c += [("f32", fold, w, "L8", p) for w in (256, 128, 64, 32, 200) for p in ALL_POINTS]
        c += [("f32", fold, w, n, "33") for w in (64, 256) for n in ("L2", "L3", "L4", "L6")]
    c += [("bf16x6", False, 256, "L8", p) for p in ALL_POINTS] + [("bf16x6", False, 256, n, "33") for n in ("L3", "L4")]  # the split ring
    c += [("bf16x6", False, w, "L8", p) for w in (64, 128) for p in ALL_POINTS]                                         # per wave
    c += [("bf16", False, 256, "L8", p) for p in ALL_POINTS] + [("bf16", False, 256, n, "33") for n in ("L3", "L4")]      # the plain ring
    c += [("bf16", False, w, "L8", p) for w in (64, 200) for p in ALL_POINTS]                        # per wave; 200: padded inside the ring
    return c


CASES = _cases()
RING = {("bf16x6", 256), ("bf16", 256), ("bf16", 200)}  # (family, width) the LDS-ring kernels serve: asserted in _kernel
RING_MAX_LAYERS = 10  # ... up to this trunk depth (RSN_RING_MAX_LAYERS, rsn_common.h: the ring kernels' LDS bias table); deeper nets run per wave


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


_dead = []


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


@contextlib.contextmanager
def _poisoned_allocators(f):
    """Saved rows, level outputs and gradient rows (folded or not) filled with NaN patterns before a kernel sees them."""
    a_saved, a_level, a_rows = f._alloc_saved, f.alloc_train_level, train_graph._alloc_gout_rows

    def rows(field, N, dev, need_input, fold):
        g, st = a_rows(field, N, dev, need_input, fold)
        _poisoned(g)
        return g, st

    f._alloc_saved = lambda N, dev, fold: _poisoned(a_saved(N, dev, fold))
    f.alloc_train_level = lambda dev, *lead: _poisoned(a_level(dev, *lead))
    train_graph._alloc_gout_rows = rows
    try:
        yield
    finally:
        del f._alloc_saved, f.alloc_train_level
        train_graph._alloc_gout_rows = a_rows


def _kernel(f, family, width):
    """The kernel family that serves this Field, asserted from the layout the library reports."""
    lay = f.train_layout()
    ring = (family, width) in RING and f.mlp_base.num_layers <= RING_MAX_LAYERS
    assert (lay["enc_cols"] == 128) == ring and (lay["sh_cols"] == 64) == ring, (family, width, lay["enc_cols"], lay["sh_cols"])
    assert lay["narrow_dtype"] == (torch.bfloat16 if (ring and family == "bf16") else f32)
    assert f.wide_dtype() == (torch.bfloat16 if family == "bf16" else f32)
    assert f.width == {32: 64, 200: 256}.get(width, width) and f.param_width == width
    return lay, ring


def _gin(n_rays, n_samples, seed, dev):
    g = torch.Generator().manual_seed(seed)
    n = n_rays * n_samples
    return {k: torch.randn(n, *s, generator=g).contiguous().to(dev)
            for k, s in (("sigma", ()), ("color", (3,)), ("pred_normals", (3,)), ("n_dot_d", ()), ("roughness", ()))}


def _rows(n, level, saved, gout, fold):
    """Host rows of one job for layer_gemm_reference.restate."""
    h = lambda t, *s: t.detach().cpu().reshape(n, *s)  # noqa: E731
    L = saved["act"].shape[0]
    rows = {"enc": h(saved["enc"], -1), "sh": h(saved["sh"], -1), "act": saved["act"].detach().cpu().reshape(L, n, -1),
            "hid": h(saved["hid"], 128), "heads": h(saved["heads"], 8), "dz_rgb": h(gout["dz_rgb"], 4), "da_mid": h(gout["da_mid"], 128),
            "dz_heads": h(gout["dz_heads"], 16), "dy": gout["dy"].detach().cpu().reshape(L, n, -1), "d_input": h(gout["d_input"])}
    if level is not None:
        rows.update({"raw_density": h(level["raw_density"]), "diff": h(level["diff"], 3), "tint": h(level["tint"], 3)})
    if not fold:
        rows.update({"bott": h(saved["bott"], -1), "d_bott": h(gout["d_bott"], -1)})
    return rows


def _judge(label, f, lay, ring, rows, layers, skips, family, fold, geometry, live=None):
    """Every record of the job and its d_input; rows [live:] (behind a device-side count) must still hold their poison."""
    P = {k: v.detach().cpu() for k, v in f.state_dict().items()}
    skip = skips[0] if skips else -1
    n = rows["enc"].shape[0]
    live = n if live is None else live
    for k, t in rows.items():
        lead = t[:, live:] if k in ("act", "dy") else t[live:]
        if lead.numel():
            it, pattern = _POISON[lead.dtype]
            assert bool((lead.contiguous().view(it) == pattern).all()), f"{label} {k}: rows behind the device-side count were written"
    cut = {k: (t[:, :live] if k in ("act", "dy") else t[:live]) for k, t in rows.items()}
    recs = G.restate(P, lay, cut, layers, skip, family, fold, ring)
    shares, failures = G.judge(label, family, recs, ring)
    print(G.report(label, shares))
    want = {f"act[{l}]" for l in range(layers)} | {f"dy[{l}]" for l in range(layers)} | {"hid", "rgb", "da_mid"}
    want |= {"head_density", "head_normals", "head_roughness", "head_diff", "head_tint"} if "raw_density" in rows else set()
    want |= set() if fold else {"bott", "d_bott"}
    assert want <= set(recs), f"{label}: records missing: {sorted(want - set(recs))}"
    geo = {k: v[: live if "sq" in geometry else live // (geometry["eb"].shape[1] - 1)] for k, v in geometry.items()}
    ref, ora = (G.d_input(P, lay, cut, layers, skip, family, geo, dt) for dt in (f64, f32))
    v = R.compare(label, "d_input", cut["d_input"], ref, ora, torch.zeros(live, dtype=torch.long), ["all"])
    print(v.report())
    return {"label": label, "shares": shares, "failures": failures, "d_input": v}


def _check(*results):
    for r in results:
        assert not r["failures"], "\n" + "\n".join(r["failures"])
        assert r["d_input"].ok, "\n" + r["d_input"].report()


def run_case(dev, family, fold, width, net, points, n_live_rays=None, nets=NETS, make_field=None, keep=False):
    """One launch pair on a frustum level -> the result of _judge (nothing asserted about the rows yet: _check).  n_live_rays: a device-side count below the buffers.
    nets: where `net` names (layers, skips); make_field(width, layers, skips): the Field instead of S._field's seed 23; keep: the result also
    carries the level, the saved rows and the Field's layout on the host ("level", "saved", "lay": tests/test_depth_skip_gpu.py)."""
    layers, skips = nets[net]
    Rn, Sn = points
    f = S._field(width, layers=layers, skips=skips, seed=23) if make_field is None else make_field(width, layers, skips)
    inp = S._rays(Rn, Sn, seed=width + layers + Rn)
    f.to(dev).train()
    f.set_mma_mode(family)
    lay, ring = _kernel(f, family, width)
    rays = (inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev))
    eb = inp["eb"].to(dev)
    gin = _gin(Rn, Sn, Rn + width, dev)
    n_dev = None if n_live_rays is None else torch.tensor([n_live_rays], dtype=torch.int32, device=dev)
    with _launching(), _poisoned_allocators(f):
        lv = f.evaluate_frustums_train(*rays, eb, n_dev=n_dev, want_normals=True, fold=fold)
        go = train_graph._field_backward(f, rays, eb, lv, gin, True, n_dev=n_dev, fold=fold)
    label = f"{family}{' folded' if fold else ''} w{width} {net} {Rn * Sn} points" + ("" if n_live_rays is None else f" ({n_live_rays * Sn} live)")
    rows = _rows(Rn * Sn, lv, lv["saved"], go, fold)
    geometry = {"o": inp["o"], "d": inp["d"], "pa": inp["pa"], "eb": inp["eb"]}
    res = _judge(label, f, lay, ring, rows, layers, skips, family, fold, geometry, None if n_live_rays is None else n_live_rays * Sn)
    if keep:
        host = lambda d: {k: v.detach().cpu() for k, v in d.items() if torch.is_tensor(v)}  # noqa: E731
        res.update({"level": host(lv), "saved": host(lv["saved"]), "lay": lay, "ring": ring, "field": f, "inputs": inp})
    return res


@pytest.mark.parametrize("family,fold,width,net,points", CASES,
                         ids=[f"{fa}{'-fold' if fo else ''}-w{w}-{n}-{p}" for fa, fo, w, n, p in CASES])
def test_every_gemm_against_fp64(dev, family, fold, width, net, points):
    _check(run_case(dev, family, fold, width, net, POINTS[points]))


COUNT_CASES = [("f32", False, 256), ("f32", True, 64), ("bf16x6", False, 256), ("bf16", False, 256)]


@pytest.mark.parametrize("family,fold,width", COUNT_CASES, ids=[f"{fa}{'-fold' if fo else ''}-w{w}" for fa, fo, w in COUNT_CASES])
def test_a_device_side_count_below_the_buffers(dev, family, fold, width):
    """60 rays x 3 samples in the buffers, 47 rays (141 points: a second tile of the 128-point tiling, ragged) live: the live rows
    pass every record, the rows behind the count keep their poison."""
    _check(run_case(dev, family, fold, width, "L8", (60, 3), n_live_rays=47))


def run_inf_case(dev, family, fold, width):
    """evaluate_reflect_train + _reflect_field_backward: a frustum level and the get_inf_color job (45 points) in one launch each
    way -> (result of the level, result of the inf job)."""
    layers, skips = NETS["L8"]
    M, Sn = 45, 2
    f = S._field(width, layers=layers, skips=skips, seed=29)
    inp = S._rays(M, Sn, seed=width + 45)
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    sq, d_inf = inf["sq"][:M].contiguous(), inf["d"][:M].contiguous()
    assert sq.shape[0] == M and float(sq.min()) < 1e-7 and float(sq.max()) > 1.0
    f.to(dev).train()
    f.set_mma_mode(family)
    lay, ring = _kernel(f, family, width)
    rays = (inp["o"].to(dev), d_inf.to(dev), inp["pa"].to(dev))  # get_inf_color reads the level's directions
    eb = inp["eb"].to(dev)
    n_dev = torch.tensor([M], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(width)
    g_color, g_bg = torch.randn(M, Sn, 3, generator=g).to(dev), torch.randn(M, 3, generator=g).to(dev)
    with _launching(), _poisoned_allocators(f):
        lv, _, inf_saved = f.evaluate_reflect_train(*rays, eb, n_dev, sq.to(dev), fold=fold)
        gouts, gout_inf = train_graph._reflect_field_backward(f, rays, sq.to(dev), [(eb, lv, g_color, Sn)], inf_saved, g_bg, n_dev, M, fold=fold)
    label = f"{family}{' folded' if fold else ''} w{width}"
    assert bool((inf_saved["sh"].cpu().float() == 0).all()), f"{label}: get_inf_color's sh rows are not exact zeros"
    lvl = _judge(label + " reflect level", f, lay, ring, _rows(M * Sn, lv, lv["saved"], gouts[0], fold), layers, skips, family, fold,
                 {"o": inp["o"], "d": d_inf, "pa": inp["pa"], "eb": inp["eb"]})
    rows = _rows(M, None, inf_saved, gout_inf, fold)
    assert bool((rows["dz_heads"] == 0).all()), f"{label}: get_inf_color has no heads gradient"
    jb = _judge(label + " get_inf_color", f, lay, ring, rows, layers, skips, family, fold, {"d": d_inf, "sq": sq})
    return lvl, jb


INF_CASES = [("f32", False, 256), ("f32", True, 256), ("bf16x6", False, 256), ("bf16", False, 256), ("bf16", False, 64)]


@pytest.mark.parametrize("family,fold,width", INF_CASES, ids=[f"{fa}{'-fold' if fo else ''}-w{w}" for fa, fo, w in INF_CASES])
def test_the_inf_job_and_its_level(dev, family, fold, width):
    """get_inf_color at 45 points (hid, heads[:, 4:7], da_mid, d sqradius and every trunk record in between) beside a reflect
    level of the same launch (its d_input is d loss / d pixel_area of the reflected rays)."""
    _check(*run_inf_case(dev, family, fold, width))
