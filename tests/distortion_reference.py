"""float64 references for the distortion loss of mip-NeRF 360 (eq. 15; include/rsn.h: rsn_distortion_forward / _backward) and the seeded
inputs tests/test_distortion_cpu.py and tests/test_distortion_gpu.py run them on.

Everything here is computed on the host from the fp32 input bits, in float64, independently of the kernels: L_ray by the literal O(S^2)
double sum, g_sigma by float64 autograd through w(sigma) (oracle/cpu_ref.py compositing, as render_reference.composite_reference does).
The O(S) prefix form the kernels use is restated here once more (loss_ray_prefix, g_w_prefix) only so that the CPU tests can hold it
against the double sum."""
import math

import torch

from oracle import cpu_ref
from tests.helpers import default_dtype
from tests.render_reference import F32_TINY, _suffix_exclusive

PLANTED = 5  # distortion_inputs plants rays 0 .. 4 (needs R >= 5)
NARROW = 1e-4  # width of the two adjacent bins that hold ray 4's weight


def distortion_seed(S):
    return 7000 + 10 * S


def distortion_inputs(R, S, seed):
    """fp32 inputs of one case, built like render_reference.composite_inputs: densities rand * 8 * (rand > 0.5), spacing bins jittered on
    [0, 1], euclidean bins on [2, 6] (the uniform sampler's map of the same bins).  g_loss_ray has mixed sign and unequal values.
    Planted rays:
      0  all sigma = 0: loss and gradient are exactly 0;
      1  sigma = 1e4 in sample 0 (plain bins): saturated, all weight in one sample, L = w^2 d / 3 and the inter-sample term is exactly 0;
      2  one zero-width bin with a finite sigma;
      3  two equal spikes (w = 1/2 each) in the first and the last sample, nothing in between: the largest inter-sample term;
      4  the weight in two adjacent bins of width NARROW: the prefix form's cancellation.
    With S == 1 rays 3 and 4 have their one sample saturated (ray 4's bin still NARROW wide)."""
    assert R >= PLANTED
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    sigma = rand(R, S) * 8.0 * (rand(R, S) > 0.5)
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    sb, eb = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, S, rand(R, S + 1))
    sb_plain, eb_plain = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, S, None)
    sb, eb = sb.clone(), eb.clone()
    g_loss = (0.25 + rand(R)) * torch.where(rand(R) < 0.4, -torch.ones(()), torch.ones(()))
    sigma[0] = 0.0
    sigma[1], sb[1], eb[1] = 0.0, sb_plain[1], eb_plain[1]
    sigma[1, 0] = 1e4
    j = S // 2
    sb[2, j + 1], eb[2, j + 1] = sb[2, j], eb[2, j]
    sigma[2, j] = 3.0
    sigma[3], sb[3], eb[3] = 0.0, sb_plain[3], eb_plain[3]
    sigma[3, S - 1] = 1e4
    if S > 1:
        sigma[3, 0] = math.log(2.0) / float(eb[3, 1] - eb[3, 0])
    sigma[4], sb[4] = 0.0, sb_plain[4]
    j = max(0, S // 2 - 1)
    sb[4, j + 1] = sb[4, j] + NARROW
    sigma[4, j] = 1e5
    if S > 1:
        sb[4, j + 2] = sb[4, j] + 2 * NARROW
        sigma[4, j] = math.log(2.0) / (4.0 * NARROW)
        sigma[4, j + 1] = 1e5
    eb[4] = sb[4] * 6.0 + (1.0 - sb[4]) * 2.0
    assert bool((sb[:, 1:] >= sb[:, :-1]).all()) and bool((eb[:, 1:] >= eb[:, :-1]).all())
    return {"sigma": sigma, "sb": sb.contiguous(), "eb": eb.contiguous(), "g_loss_ray": g_loss}


def _mid_width(sb):
    sb = sb.double()
    return (sb[..., :-1] + sb[..., 1:]) / 2, sb[..., 1:] - sb[..., :-1]


def loss_ray_terms(sb, w):
    """(inter-sample term sum_ij w_i w_j |m_i - m_j|, intra-sample term (1/3) sum_i w_i^2 d_i) per ray, by the literal double sum."""
    with default_dtype(torch.float64):
        m, d = _mid_width(sb)
        w = w.double()
        inter = (w[..., :, None] * w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum((-1, -2))
        intra = (w * w * d).sum(-1) / 3
    return inter, intra


def loss_ray_reference(sb, w):
    """L_ray [R] in float64 from the fp32 bits of the spacing bins [R,S+1] and the weights [R,S].  Every term is non-negative: the
    value is its own scale."""
    inter, intra = loss_ray_terms(sb, w)
    return inter + intra


def g_w_reference(sb, w):
    """dL_ray/dw_k = 2 sum_j w_j |m_k - m_j| + (2/3) w_k d_k by the literal sum (w may require grad: plain torch ops)."""
    m, d = _mid_width(sb)
    return 2 * (w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum(-1) + (2.0 / 3.0) * w * d


def loss_ray_prefix(sb, w):
    """The O(S) form of the kernels, in float64: 2 sum_i w_i (m_i W_<i - WM_<i) + (1/3) sum_i w_i^2 d_i on ascending bins."""
    with default_dtype(torch.float64):
        m, d = _mid_width(sb)
        w = w.double()
        ew = torch.cumsum(w, -1) - w
        ewm = torch.cumsum(w * m, -1) - w * m
        return (2 * w * (m * ew - ewm) + w * w * d / 3).sum(-1)


def g_w_prefix(sb, w):
    """dL_ray/dw_k in the O(S) form: 2 (m_k (W_<k - W_>k) - (WM_<k - WM_>k)) + (2/3) w_k d_k."""
    with default_dtype(torch.float64):
        m, d = _mid_width(sb)
        w = w.double()
        wm = w * m
        ew, ewm = torch.cumsum(w, -1) - w, torch.cumsum(wm, -1) - wm
        tw, twm = w.sum(-1, keepdim=True), wm.sum(-1, keepdim=True)
        return 2 * (m * (ew - (tw - ew - w)) - (ewm - (twm - ewm - wm))) + (2.0 / 3.0) * w * d


def weights64(inp, sigma=None):
    """The compositing weights [R,S] of the inputs in float64 (cpu_ref.weights_from_density)."""
    with default_dtype(torch.float64):
        eb = inp["eb"].double()
        s = inp["sigma"].double() if sigma is None else sigma
        return cpu_ref.weights_from_density(s[..., None], eb[:, :-1], eb[:, 1:])[..., 0]


def distortion_backward_reference(inp):
    """g_sigma [R,S] of  sum_r g_loss_ray[r] L_ray(w(sigma))  by float64 autograd through cpu_ref's compositing weights, with its scale.
      scale[k] = delta_k (|g_w[k]| T_{k+1} + sum_{i>k} |g_w[i]| w_i) + F32_TINY: the sum of the absolute values of the terms g_sigma[k]
        adds (g_w's own terms all carry the sign of g_loss_ray: |g_w| is their absolute sum), and fp32's denormal floor (the output
        is fp32: behind an opaque sample the float64 value lies below fp32's range).
    -> (g_sigma, scale, g_w)."""
    with default_dtype(torch.float64):
        sigma = inp["sigma"].double().clone().requires_grad_(True)
        eb = inp["eb"].double()
        g = inp["g_loss_ray"].double()
        w = weights64(inp, sigma)
        m, d = _mid_width(inp["sb"])
        loss = (w[..., :, None] * w[..., None, :] * (m[..., :, None] - m[..., None, :]).abs()).sum((-1, -2)) + (w * w * d).sum(-1) / 3
        (g * loss).sum().backward()
        wd = w.detach()
        delta = eb[:, 1:] - eb[:, :-1]
        x = delta * sigma.detach()
        T_next = torch.exp(-torch.cumsum(x, -1))
        gw = g[:, None] * g_w_reference(inp["sb"], wd)
        scale = delta * (gw.abs() * T_next + _suffix_exclusive(gw.abs() * wd)) + F32_TINY
    return sigma.grad, scale, gw


def g_sigma_closed_form(inp):
    """g_sigma from the rule of rsn_composite_bwd_kernel, coded on its own in float64 with plain loops over the samples:
    g_sigma[k] = delta_k (g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i)."""
    with default_dtype(torch.float64):
        sigma, eb = inp["sigma"].double(), inp["eb"].double()
        R, S = sigma.shape
        delta = eb[:, 1:] - eb[:, :-1]
        x = delta * sigma
        T = torch.ones(R, S + 1)
        for k in range(S):
            T[:, k + 1] = T[:, k] * torch.exp(-x[:, k])
        w = (1 - torch.exp(-x)) * T[:, :S]
        gw = inp["g_loss_ray"].double()[:, None] * g_w_reference(inp["sb"], w)
        out = torch.zeros(R, S)
        for k in range(S):
            out[:, k] = delta[:, k] * (gw[:, k] * T[:, k + 1] - (gw[:, k + 1:] * w[:, k + 1:]).sum(-1))
    return out
