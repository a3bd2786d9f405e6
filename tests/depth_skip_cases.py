"""The nets, the cases and the host-side checks of tests/test_depth_skip_gpu.py (trunk depths 1 .. 16 and skip positions of the field
kernels), stated once for that file, for tests/test_depth_skip_cpu.py -- which proves every case meaningful before a
GPU sees it -- and for tools/depth_skip_report.py.  Host only: no library call, no GPU.

One net per structural class, (trunk layers, live skip):
  L1      no trunk loop: the training forward's x9 loop does not run, the normal sweep peels nothing and runs its seed path alone
  L3s1    the skip is both the first trunk layer and L-2
  L5s1    skip = 1: the skip's slab round trip and the restart from b[l+1] in the first loop iteration
  L5s3    skip = L-2: in the iteration in front of `last`; the normal sweep's loop opens with the skip's encoded-input GEMM
  L7      an odd depth without a skip
  L8      the headline depth without its skip
  L8s1    the headline depth, skip at the bottom extreme
  L8s6    the headline depth, skip at the top extreme
  L9s4    the first depth above 8 (on the LDS ring in the bf16 modes at width 256)
  L10s8   the ring's maximum (RSN_RING_MAX_LAYERS), skip = L-2
  L11s4   the first depth over the ring's limit: the bf16 modes fall back to the per-wave kernels at width 256
  L16s1   the maximum depth (RSN_MAX_TRUNK_LAYERS), skip = 1
  L16s14  the maximum depth, skip = L-2

No constant here comes from a run of the kernels: BIAS_SHIFT and the integer patterns were chosen on the host, by the checks below."""
import torch

from oracle import cpu_ref
from tests import field_maths_reference as R
from tests import test_normals_seed_gpu as S
from tests.helpers import default_dtype
from tests.test_normals_x9_gpu import _integer_field

f32, f64 = torch.float32, torch.float64

NETS = {"L1": (1, ()), "L3s1": (3, (1,)), "L5s1": (5, (1,)), "L5s3": (5, (3,)), "L7": (7, ()), "L8": (8, ()), "L8s1": (8, (1,)),
        "L8s6": (8, (6,)), "L9s4": (9, (4,)), "L10s8": (10, (8,)), "L11s4": (11, (4,)), "L16s1": (16, (1,)), "L16s14": (16, (14,))}
ALL = tuple(NETS)
RING_MAX_LAYERS = 10   # RSN_RING_MAX_LAYERS (rsn_common.h)
POINTS = {"33": (11, 3), "300": (100, 3)}  # 300: a second tile of both tilings, a ring that wraps into the next tile
LIVE = (0.05, 0.95)    # a layer whose live share of units leaves this range tells little: all dead, every later record is 0 = 0


def skip_of(skips):
    return skips[0] if skips else -1


# ---------------------------------------------------------------------------------------------- 1. random fields
NARROW_F32 = ("L1", "L3s1", "L5s3", "L11s4", "L16s14")
NARROW_BF16 = ("L1", "L3s1", "L5s3", "L16s14")
# exact fp32 at width 256: unfolded and folded in one test (they must agree bit for bit upstream of the colour path)
F32_PAIRS = [(256, n, "33") for n in ALL]
# (family, fold, width, net, points) of every other case
SINGLES = ([("f32", True, 64, n, "33") for n in NARROW_F32]
           + [(fa, False, 256, n, "33") for fa in ("bf16x6", "bf16") for n in ALL]
           + [(fa, False, 256, n, "300") for fa in ("bf16x6", "bf16") for n in ("L9s4", "L10s8")]
           + [(fa, False, 64, n, "33") for fa in ("bf16x6", "bf16") for n in NARROW_BF16])


def random_cases():
    """Every (family, fold, width, net, points) of item 1, the pairs spelt out."""
    return [("f32", fold, w, n, p) for w, n, p in F32_PAIRS for fold in (False, True)] + SINGLES


def random_field(width, layers, skips, seed=23):
    """S._field's seeded Field, as test_layer_gemms_gpu.run_case builds it.  nn.Linear's default initialisation keeps about half
    the units of every layer live down to layer 15 at both widths (the biases are of the activations' size), so no weight or
    bias is rescaled: tests/test_depth_skip_cpu.py asserts the live shares of every case."""
    return S._field(width, layers=layers, skips=skips, seed=seed)


def case_rays(width, layers, points):
    """The rays test_layer_gemms_gpu.run_case draws for this case."""
    Rn, Sn = POINTS[points]
    return S._rays(Rn, Sn, seed=width + layers + Rn)


def encoded(inp):
    """fp64 encoded inputs [n, 99] of a frustum job's points (cpu_ref.ipe on field_maths_reference.gaussian)."""
    mean, var, _ = R.gaussian({**inp, "pa": inp["pa"].reshape(-1, 1)}, f64)
    with default_dtype(f64):
        return cpu_ref.ipe(cpu_ref.FieldSpec(), mean, var)


def trunk(P, layers, skip, enc, dtype=f64):
    """[pre-activation of layer l, l = 0 .. L-1], each [n, W], of the trunk on the encoded inputs (nerfstudio's MLP: the skip
    layer reads cat([enc, x]))."""
    x, out = enc.to(dtype), []
    for l in range(layers):
        w, b = P[f"mlp_base.layers.{l}.weight"].to(dtype), P[f"mlp_base.layers.{l}.bias"].to(dtype)
        xin = x if l == 0 else (torch.cat([enc.to(dtype), x], dim=1) if l == skip else x)
        z = xin @ w.t() + b
        out.append(z)
        x = torch.relu(z)
    return out


def live_shares(f, layers, skips, inp):
    """The live share of each trunk layer's units over the case's points, from the fp64 restatement."""
    P = {k: v.detach().cpu() for k, v in f.state_dict().items()}
    return [float((z > 0).double().mean()) for z in trunk(P, layers, skip_of(skips), encoded(inp))]


def assert_live(label, shares):
    for l, s in enumerate(shares):
        assert LIVE[0] < s < LIVE[1], f"{label}: layer {l} has {s:.3f} of its units live: the case tells nothing behind it"


# ---------------------------------------------------------------------------------------------- 2. integer nets
INT_NETS = tuple(n for n in ALL if n != "L1")
INT_WIDTHS = (256, 64)
EXACT = 2.0 ** 24
PIECES = 1.01 ** 2  # the magnitudes of an integer's three bf16 pieces add up to less than 1.01 times its own: both operands


def dense_layers(layers, skips):
    """The trunk layers whose W x W part holds _integer_field's small integers (eight rows a column): the skip layer and the
    layer above it, or the top layer of a net without a skip.  Every other W x W part is a signed permutation."""
    return (skips[0], skips[0] + 1) if skips else (layers - 1,)


def _permutation(width, l):
    """A signed permutation matrix [W, W] that differs from layer to layer: row i reads column (a i + c) mod W, a odd; one row in
    eight carries -1."""
    i = torch.arange(width)
    a, c = 2 * ((3 * l + 1) % (width // 2)) + 1, (37 * l + 11) % width
    w = torch.zeros(width, width)
    w[i, (a * i + c) % width] = torch.where((i + 3 * l) % 8 == 0, -1.0, 1.0)
    return w


def integer_field(width, layers, skips):
    """tests/test_normals_x9_gpu._integer_field (trunk x parts -2 .. 2 on eight rows a column, the raw-coordinate columns of the two
    encoded-input parts through -2 .. 2 with different integers in the two parts, the density row of small integers) with a signed
    permutation matrix in every W x W part but dense_layers': the magnitudes then do not grow with the depth.  The biases keep
    _integer_field's scaled random values, shifted upwards in the permutation layers (a chain of one unit a layer carries a
    gradient only while every unit on it is live: with half of them dead nothing would be left of it after fifteen layers)."""
    f = _integer_field(width, layers, skips)
    dense = dense_layers(layers, skips)
    with torch.no_grad():
        for l in range(1, layers):
            if l not in dense:
                lin = f.mlp_base.layers[l]
                lin.weight[:, lin.weight.shape[1] - width:] = _permutation(width, l)
                lin.bias.add_(BIAS_SHIFT * float(lin.bias.abs().max()))
    return f


BIAS_SHIFT = 0.3  # of the layer's largest |bias|: about two units in three keep a positive bias, and the activations a +1 row passes on keep more alive


def sweep_sums(label, P, layers, skip, masks, seed):
    """The transposed chain on integer rows: seed [n, W] is the gradient of layer L-1's pre-activation (masked already); masks[l]
    [n, W] bool.  -> (dy[l] for l = L-1 .. 0 as a list indexed by l, g_enc [n, 99]), fp64, every partial sum asserted below 2^24."""
    n = seed.shape[0]
    dy = [None] * layers
    dy[layers - 1] = seed.double()
    g_enc = torch.zeros(n, 99, dtype=f64)
    s_enc = torch.zeros(n, 99, dtype=f64)
    for l in range(layers - 1, 0, -1):
        w = P[f"mlp_base.layers.{l}.weight"].double()
        if l == skip:
            g_enc, s_enc = g_enc + dy[l] @ w[:, :99], s_enc + dy[l].abs() @ w[:, :99].abs()
            w = w[:, 99:]
        z, s = dy[l] @ w, dy[l].abs() @ w.abs()
        assert float(s.max()) * PIECES < EXACT, f"{label}: the sums of W_{l}^T may leave the exact range"
        dy[l - 1] = z * masks[l - 1].double()
    w0 = P["mlp_base.layers.0.weight"].double()
    g_enc, s_enc = g_enc + dy[0] @ w0, s_enc + dy[0].abs() @ w0.abs()
    assert float(s_enc.max()) * PIECES < EXACT, f"{label}: the encoded-input sums may leave the exact range"
    assert bool((g_enc == g_enc.round()).all())
    return dy, g_enc


def normal_sweep_case(width, net):
    """The integer field and the rays of the normal-sweep case of (width, net), with what the host can say about them before a
    launch: -> (field, rays, masks [L][n, W] of the fp64 forward, un-normalised integer gradient [n, 3])."""
    layers, skips = NETS[net]
    f, inp = integer_field(width, layers, skips), S._rays(37, 3, seed=width + layers)
    P = {k: v.detach().cpu() for k, v in f.state_dict().items()}
    masks = [z > 0 for z in trunk(P, layers, skip_of(skips), encoded(inp))]
    seed = P["field_output_density.net.weight"].double().reshape(1, width) * masks[layers - 1].double()
    _, g_enc = sweep_sums(f"normal sweep w{width} {net}", P, layers, skip_of(skips), masks, seed)
    assert float(g_enc[:, :96].abs().max()) == 0.0  # the encoded-input parts read the raw coordinates alone
    return f, inp, masks, g_enc[:, 96:99]


def assert_normal_sweep_case(label, masks, grad):
    for l, m in enumerate(masks):
        s = float(m.double().mean())
        assert LIVE[0] < s < LIVE[1], f"{label}: layer {l} mask {s:.3f} live: not a mixed mask"
    carried = float((grad.abs().amax(1) > 0).double().mean())
    assert carried > 0.9, f"{label}: only {carried:.2f} of the points carry a gradient"


def forward_field(width, layers, skips, seed):
    """tests/test_forward_x9_gpu's integer case on integer_field: every encoded-input part zero, every trunk bias an integer, layer
    0's drawn from -12 .. 12: act[0] = relu(b_0) at every point and every sum behind it is an integer."""
    f = integer_field(width, layers, skips)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for l in range(layers):
            lin = f.mlp_base.layers[l]
            if l == 0 or l in skips:
                lin.weight[:, :99] = 0.0
            lin.bias.copy_(torch.round(lin.bias))
        f.mlp_base.layers[0].bias.copy_(torch.randint(-12, 13, (width,), generator=g).float())
    return f


def forward_sums(label, f, layers, skips):
    """-> [pre-activation z_l [W]] of forward_field in fp64 (the same at every point), exactness and mixed masks asserted."""
    P = {k: v.detach().cpu() for k, v in f.state_dict().items()}
    skip, out, x = skip_of(skips), [], None
    for l in range(layers):
        w, b = P[f"mlp_base.layers.{l}.weight"].double(), P[f"mlp_base.layers.{l}.bias"].double()
        if l == 0:
            z, s = b.clone(), b.abs()
        else:
            wl = w[:, 99:] if l == skip else w
            z, s = wl @ x + b, wl.abs() @ x.abs() + b.abs()
        assert bool((z == z.round()).all()) and float(s.max()) * PIECES < EXACT, f"{label}: layer {l} is not an exact case"
        share = float((z > 0).double().mean())
        assert LIVE[0] < share < LIVE[1], f"{label}: layer {l} has {share:.3f} of its units live: not a mixed mask"
        out.append(z)
        x = torch.relu(z)
    return out


# ---------------------------------------------------------------------------------------------- 3. eval, 4. packing
EVAL_CASES = ([(m, 256, n) for m in ("f32", "bf16") for n in ("L1", "L5s1", "L5s3", "L10s8", "L11s4", "L16s14")]
              + [("bf16x6", 256, n) for n in ("L10s8", "L11s4")] + [("f32", 64, "L16s14")])
PACK_CASES = [(m, w, n) for n in ("L3s1", "L10s8", "L11s4", "L16s14") for m, w in (("f32", 64), ("bf16", 256), ("bf16x6", 256))]
