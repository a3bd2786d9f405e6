"""float64 references for depth supervision (include/rsn.h, "depth supervision": rsn_depth_loss_forward / _backward,
rsn_gather_ray_depth, rsn_depth_error) and the seeded inputs tests/test_depth_cpu.py and tests/test_depth_gpu.py run them on.

Everything here is computed on the host from the fp32 input bits, in float64, independently of the kernels.  The compositing weights
are restated here as w_k = -expm1(-x_k) exp(-X_k) (x_k = l_k sigma_k, X_k = sum_{j<k} x_j): 1 - exp(-x) in float64 loses x's digits
below 1e-8, and the term's 1 / (w + EPS) is proportional to single thin weights.  g_sigma comes from float64 autograd through that
w(sigma); the closed form the kernels use is restated once more (g_sigma_closed_form) so that the CPU tests can hold both against
finite differences.  `mutation` names one deliberate mistake (MUTATIONS): the CPU tests show that each moves a planted ray by more
than ten bounds, i.e. that the GPU tests would see it."""
import numpy as np
import torch

from oracle import cpu_ref
from reflect_sampling_nerf_amd import data
from tests.helpers import default_dtype
from tests.render_reference import EPS, F32_TINY, _suffix_exclusive

LOSS_EPS = 1e-7
DEPTH_SIGMA = 0.3   # the tests' s, in the units of the bins on [2, 6]: a few bins wide at S = 192, a fraction of the one bin at S = 1
TINY_SIGMA = 1e-20  # an s at which every Gaussian factor underflows: (m - D)^2 >= (an ulp of 2)^2 = 5.7e-14, over 2e-40
BOUND = 4 * EPS     # |got - ref64| / scale: an fp64 interior and one fp32 rounding give 2^-24; the factor 4 is headroom
PLANTED = 8         # depth_inputs plants rays 0 .. 7 (needs R >= 8)
RAY_NO_TARGET, RAY_BEFORE, RAY_BEYOND, RAY_ON_EDGE, RAY_EMPTY, RAY_SATURATED, RAY_ZERO_WIDTH, RAY_THIN = range(PLANTED)
MUTATIONS = ("no_eps", "two_s", "no_lengths", "no_mask", "bin_starts", "fp32_weights", "total_minus_prefix")


def depth_seed(S):
    return 9000 + 10 * S


def depth_inputs(R, S, seed):
    """fp32 inputs of one case: densities rand * 8 * (rand > 0.5), euclidean bins jittered on [2, 6], targets on [2.2, 5.8] with a fifth
    of the rays unsupervised (0), g_loss_ray of mixed sign and unequal size.  Planted rays:
      0  no target (D = 0): loss and gradient are exactly 0;
      1  the target before the first bin (D = 1);
      2  the target beyond the last bin (D = 7.5);
      3  the target exactly on a bin edge;
      4  an empty ray (every sigma = 0, every w = 0) with a target inside: -log(EPS) times the Gaussian mass, the largest loss;
      5  a ray saturated by its first sample (optical depth 60) with density behind it and the target in the first bins: behind the
         opaque sample the suffix sum is all there is;
      6  one zero-width bin with a finite sigma, the target next to it;
      7  a thin ray (sigma = 1e-7 everywhere): weights below EPS, where fp32 weights are off by tens of percent."""
    assert R >= PLANTED
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    sigma = rand(R, S) * 8.0 * (rand(R, S) > 0.5)
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    _, eb = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, S, rand(R, S + 1))
    _, eb_plain = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, S, None)
    eb = eb.clone()
    target = (2.2 + 3.6 * rand(R)) * (rand(R) > 0.2)
    g_loss = (0.25 + rand(R)) * torch.where(rand(R) < 0.4, -torch.ones(()), torch.ones(()))
    j = S // 2
    target[RAY_NO_TARGET] = 0.0
    target[RAY_BEFORE] = 1.0
    target[RAY_BEYOND] = 7.5
    target[RAY_ON_EDGE] = eb[RAY_ON_EDGE, j]
    sigma[RAY_EMPTY] = 0.0
    target[RAY_EMPTY] = 4.1
    eb[RAY_SATURATED] = eb_plain[RAY_SATURATED]
    sigma[RAY_SATURATED] = 2.0
    sigma[RAY_SATURATED, 0] = 60.0 / float(eb[RAY_SATURATED, 1] - eb[RAY_SATURATED, 0])
    target[RAY_SATURATED] = eb[RAY_SATURATED, min(2, S)] + 0.01
    eb[RAY_ZERO_WIDTH, j + 1] = eb[RAY_ZERO_WIDTH, j]
    sigma[RAY_ZERO_WIDTH, j] = 3.0
    target[RAY_ZERO_WIDTH] = eb[RAY_ZERO_WIDTH, j] + 0.013
    sigma[RAY_THIN] = 1e-7
    target[RAY_THIN] = 3.7
    assert bool((eb[:, 1:] >= eb[:, :-1]).all())
    return {"sigma": sigma.contiguous(), "eb": eb.contiguous(), "target": target.contiguous(), "g_loss_ray": g_loss}


class _OneMinusExpNeg(torch.autograd.Function):
    """1 - exp(-x) as -expm1(-x), with the derivative exp(-x) evaluated as such: torch's own backward of expm1 is result + 1, which
    for a large x adds 1 to -1 + exp(-x) and keeps none of exp(-x)'s digits."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return -torch.expm1(-x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.exp(-x)


def weights64(eb, sigma):
    """(w [R,S], T_next [R,S], l [R,S]) in float64: w_k = -expm1(-x_k) exp(-X_k), T_{k+1} = exp(-X_{k+1}); differentiable in sigma."""
    l = eb[:, 1:] - eb[:, :-1]
    x = l * sigma
    incl = torch.cumsum(x, -1)
    excl = torch.cat([torch.zeros_like(incl[:, :1]), incl[:, :-1]], -1)  # not incl - x: an infinite x must not poison its own T
    return _OneMinusExpNeg.apply(x) * torch.exp(-excl), torch.exp(-incl), l


def weights32(eb, sigma):
    """What rsn_composite hands out: (1 - exp(-x)) T evaluated in fp32 (the "fp32_weights" mutation reads these)."""
    l = (eb[:, 1:] - eb[:, :-1]).float()
    x = l * sigma.float()
    incl = torch.cumsum(x.double(), -1).float()
    excl = torch.cat([torch.zeros_like(incl[:, :1]), incl[:, :-1]], -1)
    return ((1.0 - torch.exp(-x)) * torch.exp(-excl)).double()


def _terms(inp, s, sigma, mutation):
    """(w, T_next, l, k) with k = [D > 0] exp(-(m - D)^2 / (2 s^2)) l the sample's kernel, under the named mutation."""
    eb, D = inp["eb"].double(), inp["target"].double()[:, None]
    s = float(np.float32(s))  # depth_sigma is a float argument of the C ABI: the fp32 input bits, like every other input
    w, T_next, l = weights64(eb, sigma)
    if mutation == "fp32_weights":
        w = weights32(inp["eb"], sigma.detach())
    pos = eb[:, :-1] if mutation == "bin_starts" else (eb[:, :-1] + eb[:, 1:]) / 2
    denom = 2 * s if mutation == "two_s" else 2 * s * s
    k = torch.exp(-(pos - D) ** 2 / denom)
    if mutation != "no_lengths":
        k = k * l
    if mutation != "no_mask":
        k = k * (D > 0)
    return w, T_next, l, k


def loss_ray_reference(inp, s=DEPTH_SIGMA, mutation=None):
    """(L_ray [R], scale [R]) in float64; scale = the sum of the absolute values of the terms + fp32's denormal floor."""
    with default_dtype(torch.float64):
        w, _, _, k = _terms(inp, s, inp["sigma"].double(), mutation)
        logw = torch.log(w if mutation == "no_eps" else w + LOSS_EPS)
        terms = torch.where(k > 0, -logw * k, torch.zeros_like(k))  # 0 * inf (the no_eps mutation off the mask) is 0
        return terms.sum(-1), terms.abs().sum(-1) + F32_TINY


def g_w_reference(inp, s=DEPTH_SIGMA, mutation=None):
    """g_loss_ray[r] dL_ray/dw_k [R,S] in float64."""
    with default_dtype(torch.float64):
        w, _, _, k = _terms(inp, s, inp["sigma"].double(), mutation)
        return -inp["g_loss_ray"].double()[:, None] * k / (w if mutation == "no_eps" else w + LOSS_EPS)


def depth_backward_reference(inp, s=DEPTH_SIGMA):
    """g_sigma [R,S] of sum_r g_loss_ray[r] L_ray(w(sigma)) by float64 autograd through weights64, with its scale
    l_k (|g_w[k]| T_{k+1} + sum_{i>k} |g_w[i]| w_i) + F32_TINY.  -> (g_sigma, scale)."""
    with default_dtype(torch.float64):
        sigma = inp["sigma"].double().clone().requires_grad_(True)
        w, T_next, l, k = _terms(inp, s, sigma, None)
        loss = (-torch.log(w + LOSS_EPS) * k).sum(-1)
        (inp["g_loss_ray"].double() * loss).sum().backward()
        gw = g_w_reference(inp, s).abs()
        scale = l * (gw * T_next.detach() + _suffix_exclusive(gw * w.detach())) + F32_TINY
    return sigma.grad, scale


def g_sigma_closed_form(inp, s=DEPTH_SIGMA, mutation=None):
    """g_sigma[k] = l_k (g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i), the rule of rsn_composite_backward, in float64; the suffix sum added
    from the far end unless the mutation takes it as total minus prefix."""
    with default_dtype(torch.float64):
        w, T_next, l, _ = _terms(inp, s, inp["sigma"].double(), mutation)
        gw = g_w_reference(inp, s, mutation)
        p = gw * w
        suffix = p.sum(-1, keepdim=True) - torch.cumsum(p, -1) if mutation == "total_minus_prefix" else _suffix_exclusive(p)
        return l * (gw * T_next - suffix)


# ------------------------------------------------------------------------------------------------------------- ray distances
def ray_depth_reference(indices, level, depths, cameras, intrinsics, euclidean):
    """t [R] in float64 from the fp32 bits: the stored value for a euclidean map, z |(X, -Y, -1)| for a z-depth, (X, Y) the pixel
    centre's normalised coordinates, undistorted by data.undistort_points (float64 Newton, the kernels' recipe) for a distorted row;
    0 for a stored 0, a level above 0 and a fisheye row with z-depths."""
    idx = np.asarray(indices, dtype=np.int64)
    out = np.zeros(len(idx), np.float64)
    for r, (i, y, x) in enumerate(idx):
        z = float(depths[i, y, x])
        if z == 0.0 or (level is not None and int(level[r]) > 0):
            continue
        if euclidean:
            out[r] = z
            continue
        row = np.asarray(cameras[i] if cameras is not None else list(intrinsics) + [0.0] * 5, dtype=np.float64)
        if len(row) == 12 and row[10] != 0.0:
            continue
        X, Y = (x + 0.5 - row[2]) / row[0], (y + 0.5 - row[3]) / row[1]
        if np.any(row[4:9] != 0.0):
            X, Y = data.undistort_points(row[:9], np.float64(X), np.float64(Y))
        out[r] = z * np.sqrt(float(X) ** 2 + float(Y) ** 2 + 1.0)
    return out


def depth_error_reference(depth, target, mask=None):
    """(sum |d - D|, sum (d - D)^2, count) over the pixels with D > 0 and a live mask byte, and the two sums' scales (themselves: every
    term is non-negative), in float64."""
    d, D = np.asarray(depth, np.float64).ravel(), np.asarray(target, np.float64).ravel()
    live = D > 0
    if mask is not None:
        live &= np.asarray(mask).ravel() != 0
    e = (d - D)[live]
    return float(np.abs(e).sum()), float((e * e).sum()), int(live.sum())
