"""The layer-by-layer rule of tests/layer_gemm_reference.py against itself, without a GPU: a float32 emulation of the training
chain (torch CPU matmul in float32; in the bf16 family with operands and stored wide rows rounded as the reference's docstring
says) stands in for the kernels and writes the rows a launch pair would.  The clean emulation has to pass every record; each
mutation -- the ways a rearranged GEMM loop goes wrong -- has to be rejected at the record it touches AND AT NO OTHER: every later
layer of the emulation consumes the mutated row, as a kernel's would, and still passes, because each record is restated on the
emulation's own input rows.  That locality is the point of the file: a failure names the broken GEMM.

The emulation shares no code with the reference (its own loops, its own mask and concatenation order, float32 throughout)."""
import pytest
import torch

from oracle import cpu_ref
from tests import field_maths_reference as R
from tests import layer_gemm_reference as G

f32, f64 = torch.float32, torch.float64
N = 96
NETS = {"L8": (8, 4), "L3": (3, -1), "L4": (4, 2)}


def _layout():
    """A slot order with padding, shuffled: 104 / 40 slots like the per-wave kernels' rows, the maps unlike any kernel's."""
    g = torch.Generator().manual_seed(5)
    enc = torch.full((104,), -1, dtype=torch.long)
    enc[torch.randperm(104, generator=g)[:99]] = torch.arange(99)
    sh = torch.full((40,), -1, dtype=torch.long)
    sh[torch.randperm(40, generator=g)[:34]] = torch.arange(34)
    return {"enc_map": enc.tolist(), "sh_map": sh.tolist(), "enc_cols": 104, "sh_cols": 40}


def _params(width, layers, skip, seed=0):
    fs = cpu_ref.FieldSpec(num_layers=layers, width=width, skip=(skip,) if skip > 0 else ())
    torch.manual_seed(seed + width + layers)
    return {k: v.float() for k, v in cpu_ref.init_params(fs).items()}


def _inputs(seed=1):
    g = torch.Generator().manual_seed(seed)
    dzh = torch.randn(N, 16, generator=g)
    dzh[:, [7, 9, 10, 11, 15]] = 0.0
    return {"enc": torch.randn(N, 99, generator=g).clamp(-1, 1), "sh": 0.3 * torch.randn(N, 34, generator=g),
            "dz_rgb": torch.randn(N, 3, generator=g), "dz_heads": dzh}


def _slots(t, cmap, cols):
    out = torch.zeros(t.shape[0], cols, dtype=t.dtype)
    for s, c in enumerate(cmap):
        if c >= 0:
            out[:, s] = t[:, c]
    return out


def emulate(P, lay, inp, layers, skip, family, fold, kernel_width, mut=None, w_c=None):
    """-> the rows of one launch pair.  mut = (name, layer) changes ONE GEMM:
    drop_k (one K term of trunk layer l dropped), swap_cols (two input columns of trunk layer l swapped), skip_order (the skip
    concatenation as [act, enc]), other_bias (trunk layer l with the bias of layer l - 1), mask_next (dy[l] masked by the mask of
    layer l + 1), kstep (dy[l - 1]: columns 32..63 of the transposed GEMM's operand taken from columns 0..31), w_not_wt (dy[l - 1]
    formed with W_l where W_l^T belongs), trunc_pack (bf16 family: every stored wide row truncated, not rounded)."""
    bf = family == "bf16"
    rnd = (lambda t: t.bfloat16().float()) if bf else (lambda t: t)
    wide = (lambda t: t.bfloat16()) if bf else (lambda t: t)
    mname, ml = mut if mut else (None, None)
    if mname == "trunc_pack":  # the stored rows cut to bf16 instead of rounded
        wide = lambda t: (t.contiguous().view(torch.int32) & -65536).view(f32).bfloat16()  # noqa: E731
    W = P["mlp_base.layers.0.weight"].shape[0]
    pad = lambda t: torch.nn.functional.pad(t, (0, kernel_width - t.shape[1]))  # noqa: E731
    lin = lambda x, w, b=None: (rnd(x) @ rnd(w).t() + (0.0 if b is None else b)).float()  # noqa: E731
    w = lambda l: P[f"mlp_base.layers.{l}.weight"]  # noqa: E731
    b = lambda l: P[f"mlp_base.layers.{l}.bias"]  # noqa: E731
    hw = lambda n: (P[f"{G.HEAD_NAMES[n]}.net.weight"], P[f"{G.HEAD_NAMES[n]}.net.bias"])  # noqa: E731
    enc = inp["enc"]
    rows = {"enc": _slots(enc, lay["enc_map"], lay["enc_cols"]), "sh": _slots(inp["sh"], lay["sh_map"], lay["sh_cols"])}
    acts, h = [], enc
    for l in range(layers):
        xin = h
        if l == skip:
            xin = torch.cat([h, enc], 1) if mname == "skip_order" else torch.cat([enc, h], 1)
        if ml == l and mname == "drop_k":
            xin = xin.clone()
            xin[:, 5] = 0.0
        if ml == l and mname == "swap_cols":
            xin = xin.clone()
            xin[:, [3, 9]] = xin[:, [9, 3]]
        bias = b(l - 1) if (ml == l and mname == "other_bias") else b(l)
        h = wide(torch.relu(lin(xin, w(l), bias))).float()
        acts.append(h)
    rows["act"] = wide(torch.stack([pad(a) for a in acts]))
    emb = acts[-1]
    rows["raw_density"] = lin(emb, *hw("density")).reshape(-1)
    heads = torch.zeros(N, 8)
    heads[:, 0:3], heads[:, 3:4] = lin(emb, *hw("normals")), lin(emb, *hw("roughness"))
    rows["diff"], rows["tint"] = torch.sigmoid(lin(emb, *hw("diff"))), torch.sigmoid(lin(emb, *hw("tint")))
    wm, bm = P["mlp_mid.layers.0.weight"], P["mlp_mid.layers.0.bias"]
    if fold:
        wc, bc = w_c if w_c is not None else G.fold_weights(P)
        hid = wide(torch.relu(lin(emb, wc, bc) + lin(inp["sh"], wm[:, :34]))).float()
    else:
        bott = wide(lin(emb, P["field_output_bottleneck.net.weight"], P["field_output_bottleneck.net.bias"])).float()
        rows["bott"] = wide(pad(bott))
        hid = wide(torch.relu(lin(torch.cat([inp["sh"], bott], 1), wm, bm))).float()
    rows["hid"] = wide(hid)
    heads[:, 4:7] = torch.sigmoid(lin(hid, P["field_output_mid.net.weight"], P["field_output_mid.net.bias"]))
    rows["heads"] = heads
    # ---- backward
    rows["dz_rgb"] = torch.nn.functional.pad(inp["dz_rgb"], (0, 1))
    rows["dz_heads"] = inp["dz_heads"]
    da = wide((hid > 0) * lin(inp["dz_rgb"], P["field_output_mid.net.weight"].t())).float()
    rows["da_mid"] = wide(da)
    if fold:
        g = lin(da, wc.t())
    else:
        db = wide(lin(da, wm[:, 34:].t())).float()
        rows["d_bott"] = wide(pad(db))
        g = lin(db, P["field_output_bottleneck.net.weight"].t())
    for n, cols in G.HEAD_COLUMNS.items():
        g = g + lin(inp["dz_heads"][:, cols], hw(n)[0].t())
    masks = [a > 0 for a in acts]
    dys = [None] * layers

    def masked(l, g):
        m = masks[l + 1] if (ml == l and mname == "mask_next") else masks[l]
        return wide(m * g).float()

    dys[layers - 1] = masked(layers - 1, g)
    for l in range(layers - 1, 0, -1):
        wl = w(l)[:, 99:] if l == skip else w(l)
        x = dys[l]
        if ml == l and mname == "kstep":
            x = x.clone()
            x[:, 32:64] = x[:, 0:32]
        g = lin(x, wl) if (ml == l and mname == "w_not_wt") else lin(x, wl.t())
        dys[l - 1] = masked(l - 1, g)
    rows["dy"] = wide(torch.stack([pad(d) for d in dys]))
    return rows


def _judge(width, net, family, fold, mut=None, kernel_width=None, w_c_emulated=None):
    layers, skip = NETS[net]
    P, lay, inp = _params(width, layers, skip), _layout(), _inputs()
    rows = emulate(P, lay, inp, layers, skip, family, fold, kernel_width or width, mut, w_c_emulated)
    recs = G.restate(P, lay, rows, layers, skip, family, fold)
    shares, failures = G.judge(f"w{width} {net} {family} fold={fold} {mut}", family, recs)
    print(G.report(f"w{width} {net} {family} fold={fold} {mut}", shares))
    return recs, shares, failures


FAMILY_CASES = [("f32", False), ("f32", True), ("bf16x6", False), ("bf16", False)]


@pytest.mark.parametrize("family,fold", FAMILY_CASES)
@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("width", [64, 256])
def test_the_clean_emulation_passes_every_record(width, net, family, fold):
    recs, shares, failures = _judge(width, net, family, fold)
    layers = NETS[net][0]
    expect = {f"act[{l}]" for l in range(layers)} | {f"dy[{l}]" for l in range(layers)} | {
        "head_density", "head_normals", "head_roughness", "head_diff", "head_tint", "hid", "rgb", "da_mid"}
    if not fold:
        expect |= {"bott", "d_bott"}
    assert set(recs) == expect
    assert not failures, "\n".join(failures)
    assert all(float(r.S.max()) > 0 for r in recs.values())


def test_padded_units_are_judged_as_exact_zeros():
    """Width 200 inside a 256-wide kernel: the padded columns have S = 0, so B = 0; a non-zero there is a failure."""
    recs, _, failures = _judge(200, "L8", "f32", False, kernel_width=256)
    assert not failures, "\n".join(failures)
    assert recs["act[3]"].ref.shape[1] == 256 and float(recs["act[3]"].S[:, 200:].abs().max()) == 0.0
    layers, skip = NETS["L8"]
    P, lay, inp = _params(200, layers, skip), _layout(), _inputs()
    rows = emulate(P, lay, inp, layers, skip, "f32", False, 256)
    rows["dy"][2, 7, 230] = 1e-30
    _, failures = G.judge("poked", "f32", G.restate(P, lay, rows, layers, skip, "f32"))
    assert len(failures) == 1 and "record dy, layer 2: point 7, column 230" in failures[0]


# (mutation, layer, the one record that has to fail); L8 skip 4
MUTATIONS = [(("drop_k", 2), "act[2]"), (("drop_k", 0), "act[0]"), (("swap_cols", 5), "act[5]"), (("swap_cols", 4), "act[4]"),
             (("skip_order", 4), "act[4]"), (("other_bias", 3), "act[3]"), (("mask_next", 2), "dy[2]"), (("mask_next", 6), "dy[6]"),
             (("kstep", 3), "dy[2]"), (("kstep", 4), "dy[3]"), (("w_not_wt", 6), "dy[5]"), (("w_not_wt", 1), "dy[0]")]


@pytest.mark.parametrize("family,fold", FAMILY_CASES)
@pytest.mark.parametrize("mut,where", MUTATIONS, ids=[f"{m[0]}{m[1]}" for m, _ in MUTATIONS])
@pytest.mark.parametrize("width", [64, 256])
def test_a_mutation_is_rejected_at_its_own_record_and_at_no_other(width, mut, where, family, fold):
    recs, shares, failures = _judge(width, "L8", family, fold, mut)
    bad = {k for k, v in shares.items() if any(f"record {recs[k].name}, layer {recs[k].layer}:" in f for f in failures)}
    assert bad == {where}, f"{mut}: rejected at {sorted(bad)}, expected {where} alone\n" + "\n".join(failures)


@pytest.mark.parametrize("width", [64, 256])
def test_a_truncating_pack_is_rejected_at_every_row_stored_as_bf16(width):
    """The bf16 term of the bound is HALF a bf16 ulp, what round-to-nearest-even leaves: rows cut to bf16 instead (up to a whole
    ulp off) fail at every record the kernels store as bf16 -- and at no record kept in fp32, whose inputs are those rows."""
    recs, shares, failures = _judge(width, "L8", "bf16", False, ("trunc_pack", None))
    bad = {k for k in recs if any(f"record {recs[k].name}, layer {recs[k].layer}:" in f for f in failures)}
    assert bad == {k for k, r in recs.items() if r.stored_bf16} and len(bad) == 20
    assert all(1.0 < shares[k] <= 2.0 for k in bad)


@pytest.mark.parametrize("width", [64, 256])
def test_a_folded_w_c_formed_in_fp32_passes(width):
    """The rule does NOT see W_c = W_mx W_b formed in fp32 instead of fp64, and the arithmetic says so: an fp32 product sum
    of W terms moves an entry of W_c by at most W 2^-24 sum |w_mx| |w_b|, by ~sqrt(W) 2^-24 of it in a blocked sum of random
    signs, i.e. a few ulp of |W_c|; the pre-activation then moves by a few 2^-24 of sum |W_c| |act| -- well inside K u S with
    K = W + 36.  (What the packing must not get wrong is checked where W_c is produced: tests/test_fold_bottleneck_gpu.py.)"""
    layers, skip = NETS["L8"]
    P = _params(width, layers, skip)
    wm, wb = P["mlp_mid.layers.0.weight"], P["field_output_bottleneck.net.weight"]
    w32 = (wm[:, 34:] @ wb, P["mlp_mid.layers.0.bias"] + wm[:, 34:] @ P["field_output_bottleneck.net.bias"])
    assert not torch.equal(w32[0], G.fold_weights(P)[0])
    _, shares, failures = _judge(width, "L8", "f32", True, w_c_emulated=w32)
    assert not failures, "\n".join(failures)
    assert shares["hid"] < 0.5 and shares["dy[7]"] < 0.5


def test_the_constants_are_the_derived_ones():
    assert G.U == 2.0 ** -23 and G.HALF_ULP_BF16 == 2.0 ** -8
    # half a bf16 ulp: what round-to-nearest-even leaves, attained just above a power of two
    v = torch.tensor([0.5058791, 1.0, 1.99, 3e-5, 0.0], dtype=f64)
    assert G.half_ulp_bf16(v).tolist() == [2.0 ** -9, 2.0 ** -8, 2.0 ** -8, 2.0 ** -24, 0.0]
    x = torch.rand(100000, generator=torch.Generator().manual_seed(1)) * 4
    e = (x.bfloat16().double() - x.double()).abs()
    assert bool((e <= G.half_ulp_bf16(x.double())).all()) and bool((e > 2.0 ** -9 * x.double()).any())
    assert 2 * 2.0 ** -24 <= G.C_X6 < 3 * 2.0 ** -24
    # the split of rsn_gemm_loops.h on random values: pieces to nearest even, the dropped part within C_X6 |w| |x|
    g = torch.Generator().manual_seed(0)
    w, x = torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g)

    def split(v):
        a = v.bfloat16().float()
        b = (v - a).bfloat16().float()
        return a, b, (v - a - b).bfloat16().float()

    (w1, w2, w3), (x1, x2, x3) = split(w), split(x)
    kept = sum(p.double() * q.double() for p, q in ((w1, x1), (w1, x2), (w2, x1), (w1, x3), (w2, x2), (w3, x1)))
    assert torch.equal(w1 + w2 + w3, w) and torch.equal(x1 + x2 + x3, x)  # no residual
    dropped = (w.double() * x.double() - kept).abs() / (w.double() * x.double()).abs()
    assert float(dropped.max()) <= G.C_X6 and float(dropped.max()) > G.C_X6 / 16  # derived, and not idle


def test_d_input_restatement_is_autograd_through_the_encoding():
    """layer_gemm_reference.d_input in fp64 against fp64 autograd of sum(g_enc . IPE(mean, var(pixel_area))) with the mean held
    constant, and the get_inf_color form against autograd through var = 0.6 sq (1 - d^2)."""
    layers, skip = NETS["L8"]
    P, lay = _params(64, layers, skip), _layout()
    geo = {k: v for k, v in R.build_inputs(n_area=2, n_bins=2, n_axis=2, n_len=2).items() if k in ("o", "d", "pa", "eb")}
    S = geo["eb"].shape[1] - 1
    n = geo["o"].shape[0] * S
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(layers, n, 64, generator=g)
    freqs = R.frequencies()

    def chain(mean32, var):
        enc = torch.cat([R.ipe_rows(mean32, var, freqs, f64), mean32.double()], dim=1)
        g_enc = dy[0].double() @ P["mlp_base.layers.0.weight"].double() + dy[skip].double() @ P[f"mlp_base.layers.{skip}.weight"].double()[:, :99]
        return enc, (g_enc * enc).sum()

    pa = geo["pa"].double().requires_grad_(True)
    mean, var, _ = R.gaussian({**geo, "pa": pa}, f64)
    enc, loss = chain(mean.detach().float(), var)
    (ref,) = torch.autograd.grad(loss, pa)  # per ray: the sum over its samples
    rows = {"dy": dy, "enc": _slots(enc.detach(), lay["enc_map"], 104)}  # (the fp64 features: pure algebra, no float32 rounding)
    got = G.d_input(P, lay, rows, layers, skip, "f32", geo, f64).reshape(-1, S).sum(1)
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max()) and float(ref.abs().max()) > 0
    inf = R.build_inf_inputs(per_decade=2)
    m = inf["d"].shape[0]
    sq = inf["sq"].double().requires_grad_(True)
    mean, var = R.inf_gaussian({"d": inf["d"], "sq": sq}, f64)
    dy = torch.randn(layers, m, 64, generator=g)
    enc, loss = chain(mean.detach().float(), var)
    (ref,) = torch.autograd.grad(loss, sq)
    rows = {"dy": dy, "enc": _slots(enc.detach(), lay["enc_map"], 104)}
    got = G.d_input(P, lay, rows, layers, skip, "f32", {"d": inf["d"], "sq": inf["sq"]}, f64)
    assert float((got - ref).abs().max()) <= 1e-9 * float(ref.abs().max()) and float(ref.abs().max()) > 0
