"""Every GEMM of a training launch, restated in fp64 ON THE KERNEL'S OWN INPUT ROWS, and the rule its output row is judged by.

A training forward saves the operand of every GEMM (rsn_field_saved: enc, act[l], bott, sh, hid, heads; raw_density among the
outputs) and a backward sweep writes every layer's gradient row (rsn_field_grads_out: dz_rgb, da_mid, d_bott, dz_heads, dy[l],
d_input).  restate() takes those rows on the host and returns one Record per GEMM: the fp64 result `ref` of the GEMM on the row
the kernel wrote in front of it, and the scale S = sum_k |w_k| |x_k| + |b| of the same shape.  Nothing propagates from one record
to the next, so a failure names the GEMM that is wrong; no ReLU flip is an excuse (the masks are the kernel's own act > 0, the
bit-packed ReLU words are deliberately not decoded: a wrong bit is a gradient entry that should be zero and is not, or the
reverse) and no point is left out.

Users: tests/test_layer_gemms_cpu.py (the rule against a float32 emulation of the chain and the mutations it has to reject at
their own record) and tests/test_layer_gemms_gpu.py (the three training kernel families).

Families ("f32", "bf16x6", "bf16") and what each one's MFMA operands are:
  f32      the fp32 rows and the fp32 weights themselves (v_mfma_f32_32x32x2_f32).  fold=True: W_c = W_mid[:, 34:] W_b and
           b_c = b_mid + W_mid[:, 34:] b_b formed in fp64 and rounded ONCE to fp32, as rsn_fold_kernel (rsn_pack.hip) leaves them
           (README).
  bf16x6   the same fp32 rows and weights, each split into three bf16 pieces (rsn_gemm_loops.h: split8; rsn_pack.hip: the layout-2
           branch of the pack kernel and the split copy kernel; rsn_field_x6_train.hip: the pack2<false> chain), six of the nine piece
           products kept (mma16).  Every piece is a round-to-nearest-even conversion, `(__bf16)x` / v_cvt_pk_bf16_f32.
  bf16     ONE bf16 piece a side, fp32 accumulation from an fp32 bias.  Weights: `(__bf16)v` in the pack kernel of rsn_pack.hip
           (round to nearest even).  Rows: the wide rows (act, bott, hid, dy, d_bott, da_mid) are stored as bf16 and read back
           as stored -- rsn_ring16.h: pack2 (v_cvt_pk_bf16_f32 through __builtin_convertvector, nearest even) on the ring,
           rsn_gemm_loops.h: put4 / sv_put `(__bf16)v` per wave, and the per-wave GEMM rounds its fp32 LDS copy by split8<1>, the same
           conversion.  Rows kept in fp32 are rounded where the operand is formed: enc / sh of the per-wave instantiation
           (rsn_gemm_loops.h: split8<1> in gemm_bf16), dz_heads / dz_rgb of both sweeps (rsn_field_bf16_train.hip: pack2<false> into
           XH / X0 of rsn_field_bf16_bwd_kernel; split8<1> per wave) -- nearest even everywhere.  The reference therefore
           applies ONE rounding, to_bf16 below, to every operand of this family (it is the identity on a row that is bf16 already).

The rule, per entry, u = 2^-23, K = the GEMM's inner length + 2 (bias, final add):
    B = K u S                                        f32
    B = K u S + C_X6 S                               bf16x6
    B = K u S~ + h(|ref| + K u S~)                   bf16, S~ on the rounded operands; h = 0 on a row stored in fp32
K u S covers fp32 accumulation of the K products in any order, whatever the MFMA's internal rounding: n additions lose at most
(n - 1) 2^-24 of the sum of magnitudes, and u is twice that unit.  h(v) covers the bf16 rounding of the stored row: the fp32
accumulator a is within K u S~ of ref and the row holds bf16(a), to nearest even (pack2 / put4, above), so it is within HALF A
BF16 ULP of a: h(v) = 2^-8 2^floor(log2 v), between 2^-9 v (v at the top of its binade) and 2^-8 v (v a power of two) -- a
truncating pack would need the whole ulp, twice that.  (A flat 2^-9 |ref| is the top-of-binade value only: a correctly rounded
0.5058 is 0.5078, 2^-9 away and 2^-8.03 relative; tests/test_layer_gemms_cpu.py holds that case.)  h is taken of |ref| + K u S~
because a and ref may lie either side of a power of two.
ReLU is 1-Lipschitz, so |got - relu(ref)| <= B is the whole rule of an activated row, kink or not, and the same holds for a gradient row masked by the kernel's own act > 0 (B = 0 where the mask is 0:
such an entry must be an exact zero, as must every entry of a zero-padded unit).  diff, tint and the mid colour heads[:, 4:7] leave
the kernels through their sigmoid (the raw values are not kept): sigmoid is 1/4-Lipschitz, so B / 4 plus the family's sigmoid
allowance (sigmoid_allowance).

d_input is not one GEMM (two transposed GEMMs, the IPE's variance chain and the Gaussian's): d_input() restates it in a given
dtype and the callers judge it with field_maths_reference.compare, float32 restatement as the oracle.

No constant in this file comes from a run of the kernels."""
import torch

from tests import field_maths_reference as R

U = 2.0 ** -23
# bf16x6 (rsn_gemm_loops.h: split8<3>, mma16): x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), all to nearest even, 8 significant
# bits each.  For |x| in [2^e, 2^(e+1)): |x - x1| <= 2^(e-8) (half a bf16 ulp), so |x2| <= 2^-8 |x|; x - x1 is a multiple of the fp32
# ulp 2^(e-23) and x2 keeps its leading 8 bits to within 2^(e-16), so |x3| <= 2^-16 |x|; what is left is a multiple of 2^(e-23) below
# 2^(e-16), which fits the 8 bits of x3: the split has NO residual (barring underflow below 2^-126), x = x1 + x2 + x3.  The same
# for w.  mma16 keeps w1x1, w1x2, w2x1, w1x3, w2x2, w3x1 and drops   w2 x3 + w3 x2 + w3 x3,   at most
# (2^-24 + 2^-24 + 2^-32) |w| |x| = 2^-23 (1 + 2^-9) |w| |x|: two of the 2^-24 of include/rsn.h ("dropped terms <= 2^-24 relative").
# (Every piece product is exact in fp32; the extra accumulation steps of the six products are inside K u S: one fp32 rounding
# per v_mfma_f32_32x32x16_bf16, 6 K / 16 of them.)
C_X6 = 2.0 ** -23 * (1.0 + 2.0 ** -9)
HALF_ULP_BF16 = 2.0 ** -8  # of the power of two at or below the value: pack2 / put4 round to nearest even (a truncating pack: 2^-7)
HEAD_COLUMNS = {"density": [0], "normals": [1, 2, 3], "diff": [4, 5, 6], "roughness": [8], "tint": [12, 13, 14]}  # dz_heads, include/rsn.h
HEAD_NAMES = {"density": "field_output_density", "normals": "field_output_normals", "diff": "field_output_diff",
              "roughness": "field_output_roughness", "tint": "field_output_tint"}
FAMILIES = ("f32", "bf16x6", "bf16")


def to_bf16(t):
    """Round to nearest even to bf16, returned in t's dtype (float32 / float64 holding float32 values)."""
    return t.float().bfloat16().to(t.dtype)


class Record:
    """One GEMM: got [n, cols] (the kernel's row, fp64), ref / S [n, cols] fp64 (ref AFTER the activation or mask), K, layer (or
    None), kind: "linear", "relu", "masked" or "sigmoid", stored_bf16: whether the kernel rounds the row to bf16 when it stores it."""

    def __init__(self, name, layer, got, ref, S, K, kind, stored_bf16):
        self.name, self.layer, self.K, self.kind, self.stored_bf16 = name, layer, K, kind, stored_bf16
        n = ref.shape[0]
        self.got, self.ref, self.S = got.double().reshape(n, -1), ref.double().reshape(n, -1), S.double().reshape(n, -1)
        assert self.got.shape == self.ref.shape == self.S.shape, (name, self.got.shape, self.ref.shape, self.S.shape)

    @property
    def label(self):
        return self.name if self.layer is None else f"{self.name}[{self.layer}]"


def sigmoid_allowance(family, ring, ref_raw):
    """What the family's sigmoid may add to diff / tint, elementwise, from the raw fp64 value.  Exact kernels (sigmoid_f,
    rsn_field_common.h): the fp32 rule of field_maths_reference.compare -- FACTOR x the worst error of torch's float32 sigmoid on
    the same raw values, plus one ulp of a value below 1.  The plain ring's fast_sigmoid: relative 2 (2e-7 + 8e-8 |x|), the
    FAST_SIGMOID of tests/test_field_maths_gpu.py (formula error with correctly rounded exp2 / rcp, doubled for 1-ulp hardware)."""
    s = torch.sigmoid(ref_raw)
    if family == "bf16" and ring:
        return 2.0 * (2e-7 + 8e-8 * ref_raw.abs()) * s
    ora = (torch.sigmoid(ref_raw.float()).double() - s).abs().max()
    return torch.full_like(s, R.FACTOR * float(ora) + R.ULP)


def half_ulp_bf16(v):
    """Half a bf16 ulp (8 significant bits) of the non-negative fp64 values v: 2^-8 2^floor(log2 v); 0 at 0."""
    m, e = torch.frexp(v)  # v = m 2^e, m in [0.5, 1)
    return torch.where(v > 0, torch.ldexp(torch.full_like(v, HALF_ULP_BF16), e - 1), torch.zeros_like(v))


def bound(rec, family, ring=False):
    """The per-entry bound B of the module docstring for one record."""
    B = rec.K * U * rec.S
    if family == "bf16x6":
        B = B + C_X6 * rec.S
    elif family == "bf16" and rec.stored_bf16:
        B = B + half_ulp_bf16(rec.ref.abs() + B)
    if rec.kind == "sigmoid":
        B = B / 4.0 + sigmoid_allowance(family, ring, rec.raw)
    return B


def columns(rows, cmap, n_cols, dtype):
    """Rows in the kernel's slot order -> [n, n_cols] in the reference's column order (padding slots ignored)."""
    cmap = torch.tensor(cmap)
    live = (cmap >= 0).nonzero().flatten()
    assert sorted(cmap[live].tolist()) == list(range(n_cols)), f"the slot map does not cover the {n_cols} columns once"
    out = torch.zeros(rows.shape[0], n_cols, dtype=dtype)
    out[:, cmap[live]] = rows[:, live].to(dtype)
    return out


def fold_weights(P):
    """W_c [128, W], b_c [128] of RSN_MMA_F32_FOLDED: fp64 products and sums, ONE rounding to fp32 (rsn_fold_kernel, rsn_pack.hip;
    the restatement of tests/test_fold_bottleneck_cpu.py: wc = wmx @ wb, bc = bm + wmx @ bb)."""
    wm, bm = P["mlp_mid.layers.0.weight"].double(), P["mlp_mid.layers.0.bias"].double()
    wb, bb = P["field_output_bottleneck.net.weight"].double(), P["field_output_bottleneck.net.bias"].double()
    wmx = wm[:, 34:]
    return (wmx @ wb).float(), (bm + wmx @ bb).float()


class _Net:
    """The parameters as the family's operands, in `dtype`."""

    def __init__(self, P, layers, skip, family, fold, dtype, w_c=None):
        assert family in FAMILIES and not (fold and family != "f32"), (family, fold)
        self.L, self.skip, self.family, self.fold, self.dtype = layers, skip, family, fold, dtype
        self.rnd = to_bf16 if family == "bf16" else (lambda t: t)
        w = lambda k: self.rnd(P[k].detach().cpu().to(dtype))  # noqa: E731
        b = lambda k: P[k].detach().cpu().to(dtype)  # noqa: E731  (the bias starts the fp32 accumulator: never rounded)
        self.W = [w(f"mlp_base.layers.{l}.weight") for l in range(layers)]
        self.b = [b(f"mlp_base.layers.{l}.bias") for l in range(layers)]
        self.Wp = self.W[0].shape[0]
        self.heads = {k: (w(f"{n}.net.weight"), b(f"{n}.net.bias")) for k, n in HEAD_NAMES.items()}
        self.W_b, self.b_b = w("field_output_bottleneck.net.weight"), b("field_output_bottleneck.net.bias")
        self.W_mid, self.b_mid = w("mlp_mid.layers.0.weight"), b("mlp_mid.layers.0.bias")
        self.W_rgb, self.b_rgb = w("field_output_mid.net.weight"), b("field_output_mid.net.bias")
        if fold:
            wc, bc = fold_weights(P) if w_c is None else w_c
            self.W_c, self.b_c = wc.to(dtype), bc.to(dtype)

    def x_part(self, l):
        """W_{l,x}: the part of layer l's weight that multiplies act[l-1] (at the skip layer: behind the 99 encoded columns)."""
        return self.W[l][:, 99:] if l == self.skip else self.W[l]


def _affine(x, w, b=None):
    """-> (x w^T + b, |x| |w|^T + |b|)"""
    z, s = x @ w.t(), x.abs() @ w.abs().t()
    return (z, s) if b is None else (z + b, s + b.abs())


def _pad(t, cols):
    return t if t.shape[1] == cols else torch.nn.functional.pad(t, (0, cols - t.shape[1]))


def restate(P, lay, rows, layers, skip, family, fold=False, ring=False, dtype=torch.float64, w_c=None):
    """P: the Field's state_dict; lay: its train_layout() (enc_map / sh_map); rows: host tensors of ONE job of one launch pair --
    enc [n, enc_cols], sh [n, sh_cols], act [L, n, W], hid [n, 128], heads [n, 8], bott [n, W] (unfolded), and whichever of
    raw_density [n], diff / tint [n, 3], dz_rgb [n, 4], da_mid [n, 128], d_bott [n, W], dz_heads [n, 16], dy [L, n, W] the job
    has: a record is returned for every GEMM whose input and output rows are there.  skip: the live skip layer or -1.  ring: the
    family's LDS-ring kernel wrote the rows (only the sigmoid allowance depends on it).  w_c: (W_c, b_c) to use instead of
    fold_weights (tests/test_layer_gemms_cpu.py).  -> {label: Record}."""
    net = _Net(P, layers, skip, family, fold, dtype, w_c)
    L, Wp, rnd, bf = layers, net.Wp, net.rnd, family == "bf16"
    x = lambda t: rnd(t.detach().cpu().to(dtype))  # noqa: E731  an operand row
    enc = rnd(columns(rows["enc"].detach().cpu(), lay["enc_map"], 99, dtype))
    sh = rnd(columns(rows["sh"].detach().cpu(), lay["sh_map"], 34, dtype))
    act = rows["act"].detach().cpu()
    Wk = act.shape[2]
    out = {}

    def add(name, layer, got, ref, S, K, kind, stored_bf16, raw=None):
        rec = Record(name, layer, got.detach().cpu(), ref, S, K, kind, stored_bf16)
        rec.raw = raw
        out[rec.label] = rec

    # ---------------------------------------------------------------- forward
    for l in range(L):
        xin = enc if l == 0 else x(act[l - 1][:, :Wp])
        if l == skip:
            xin = torch.cat([enc, xin], dim=1)  # encoded inputs first (nerfstudio's MLP)
        z, s = _affine(xin, net.W[l], net.b[l])
        add("act", l, act[l], _pad(torch.relu(z), Wk), _pad(s, Wk), xin.shape[1] + 2, "relu", bf)
    emb = x(act[L - 1][:, :Wp])
    hd = rows["heads"].detach().cpu()
    frustum = rows.get("raw_density") is not None  # (get_inf_color has no head outputs: its job brings no raw_density)
    for name, got in (("density", rows.get("raw_density")), ("normals", hd[:, 0:3]), ("roughness", hd[:, 3])):
        if frustum:
            z, s = _affine(emb, *net.heads[name])
            add("head_" + name, None, got.reshape(got.shape[0], -1), z, s, Wp + 2, "linear", False)
    for name in ("diff", "tint"):
        if frustum:
            z, s = _affine(emb, *net.heads[name])
            add("head_" + name, None, rows[name].reshape(-1, 3), torch.sigmoid(z), s, Wp + 2, "sigmoid", False, raw=z)
    if fold:
        z, s = _affine(emb, net.W_c, net.b_c)
        z2, s2 = _affine(sh, net.W_mid[:, :34])
        add("hid", None, rows["hid"], torch.relu(z + z2), s + s2, Wp + 34 + 2, "relu", bf)
    else:
        z, s = _affine(emb, net.W_b, net.b_b)
        add("bott", None, rows["bott"], _pad(z, Wk), _pad(s, Wk), Wp + 2, "linear", bf)
        xin = torch.cat([sh, x(rows["bott"][:, :Wp])], dim=1)  # mlp_mid reads [sh, bottleneck] (oracle/cpu_ref.mid_color)
        z, s = _affine(xin, net.W_mid, net.b_mid)
        add("hid", None, rows["hid"], torch.relu(z), s, Wp + 34 + 2, "relu", bf)
    hid = x(rows["hid"])
    z, s = _affine(hid, net.W_rgb, net.b_rgb)
    # saved.heads[:, 4:7] holds the mid colour AFTER its sigmoid (colour_out, rsn_field_common.h; head_grad_inputs reads it as such)
    add("rgb", None, hd[:, 4:7], torch.sigmoid(z), s, 128 + 2, "sigmoid", False, raw=z)
    # ---------------------------------------------------------------- backward
    if rows.get("da_mid") is None:
        return out
    m_hid = (rows["hid"].detach().cpu().double() > 0).to(dtype)
    mask = lambda l: (act[l][:, :Wp].double() > 0).to(dtype)  # noqa: E731
    z, s = _affine(x(rows["dz_rgb"][:, :3]), net.W_rgb.t())
    add("da_mid", None, rows["da_mid"], m_hid * z, m_hid * s, 3 + 2, "masked", bf)
    da = x(rows["da_mid"])
    if fold:
        z, s = _affine(da, net.W_c.t())
        K = 128
    else:
        z, s = _affine(da, net.W_mid[:, 34:].t())
        add("d_bott", None, rows["d_bott"], _pad(z, Wk), _pad(s, Wk), 128 + 2, "linear", bf)
        z, s = _affine(x(rows["d_bott"][:, :Wp]), net.W_b.t())
        K = Wp
    if rows.get("dz_heads") is not None:
        dzh = x(rows["dz_heads"])
        for name, cols in HEAD_COLUMNS.items():
            z2, s2 = _affine(dzh[:, cols], net.heads[name][0].t())
            z, s, K = z + z2, s + s2, K + len(cols)
    dy = rows["dy"].detach().cpu()
    m = mask(L - 1)
    add("dy", L - 1, dy[L - 1], _pad(m * z, Wk), _pad(m * s, Wk), K + 2, "masked", bf)
    for l in range(L - 1, 0, -1):
        z, s = _affine(x(dy[l][:, :Wp]), net.x_part(l).t())
        m = mask(l - 1)
        add("dy", l - 1, dy[l - 1], _pad(m * z, Wk), _pad(m * s, Wk), Wp + 2, "masked", bf)
    return out


def d_input(P, lay, rows, layers, skip, family, geometry, dtype):
    """d loss / d pixel_area (geometry = {"o", "d", "pa", "eb"}: rays of [R, S] samples) or d sqradius (geometry = {"d", "sq"}:
    get_inf_color) of every point, in `dtype`, from the kernel's own dy[0], dy[skip] and saved enc rows:
      g_enc = W_0^T dy[0] + W_{skip,enc}^T dy[skip]                                      (the family's operands, see restate)
      d loss / d var_c = -1/2 sum_f f^2 (g_sin(c, f) sin feature + g_cos(c, f) cos feature)   (fold_enc, rsn_field_bf16_train.hip)
      frustum: sum_c d loss / d var_c  d var_c / d pixel_area by autograd through field_maths_reference.gaussian;
      inf:     var_c = 0.6 sq (1 - d_c^2) (field_maths_reference.inf_gaussian; get_inf_color's SH inputs are zeros, so
               nothing reaches sqradius through them)."""
    net = _Net(P, layers, skip, family, False, dtype)
    Wp, rnd = net.Wp, net.rnd
    dy = rows["dy"].detach().cpu()
    g_enc = rnd(dy[0][:, :Wp].to(dtype)) @ net.W[0]
    if skip > 0:
        g_enc = g_enc + rnd(dy[skip][:, :Wp].to(dtype)) @ net.W[skip][:, :99]
    feat = columns(rows["enc"].detach().cpu(), lay["enc_map"], 99, dtype)
    f2 = (R.frequencies().to(dtype) ** 2).repeat(3)
    n = feat.shape[0]
    dvar = -0.5 * ((g_enc[:, :48] * feat[:, :48] + g_enc[:, 48:96] * feat[:, 48:96]) * f2).reshape(n, 3, 16).sum(-1)
    if "sq" in geometry:
        d = geometry["d"].to(dtype)
        return (dvar * (0.6 * (1.0 - d * d))).sum(-1)
    S = geometry["eb"].shape[1] - 1
    eb = geometry["eb"].to(dtype)
    pa = geometry["pa"].to(dtype).reshape(-1).repeat_interleave(S).requires_grad_(True)
    one = {"o": geometry["o"].repeat_interleave(S, 0), "d": geometry["d"].repeat_interleave(S, 0), "pa": pa,
           "eb": torch.stack([eb[:, :-1].reshape(-1), eb[:, 1:].reshape(-1)], dim=1)}  # every point a ray of one sample
    var = R.gaussian(one, dtype)[1]
    (g,) = torch.autograd.grad((var * dvar.detach()).sum(), pa)
    return g.detach()


def judge(label, family, records, ring=False):
    """-> (shares {record label: worst |err| / B, B == 0 entries counted as 0 when exact and inf when not}, failures [str]).
    Every entry of every row is judged; a failure names family, record (layer), point, column, |err|, B and S."""
    shares, failures = {}, []
    for key, rec in records.items():
        B = bound(rec, family, ring)
        err = (rec.got - rec.ref).abs().nan_to_num(nan=float("inf"), posinf=float("inf"))
        bad = err > B
        share = torch.where(B > 0, err / B.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        shares[key] = float(share.max()) if share.numel() else 0.0
        if bool(bad.any()):
            i = int(torch.where(bad, share, torch.full_like(share, -1.0)).argmax())
            p, c = divmod(i, err.shape[1])
            failures.append(f"[{label}] family {family}, record {rec.name}, layer {rec.layer}: point {p}, column {c}: |err| {float(err[p, c]):.3e} "
                            f"> B {float(B[p, c]):.3e} (S {float(rec.S[p, c]):.3e}, ref {float(rec.ref[p, c]):.6e}, got {float(rec.got[p, c]):.6e}); "
                            f"{int(bad.sum())} of {bad.numel()} entries beyond B")
    return shares, failures


def report(label, shares):
    return f"[{label}] worst |err| / B per record: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items())
