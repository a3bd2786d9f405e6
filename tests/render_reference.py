"""float64 references for the ray-level kernels around the field (compositing and its backward, the reflect setup / combine and their
backwards, the per-ray losses, ray and column sums), and the seeded inputs tests/test_render_ops_gpu.py runs them on.

Everything here is computed on the host from the fp32 input bits, in float64 (tests.helpers.default_dtype), independently of the
kernels: compositing through oracle/cpu_ref.py and float64 autograd, the other entry points from the formulas in include/rsn.h.
tests/test_render_reference_cpu.py checks the compositing gradients against the closed form and the exclusion caps on these inputs."""
import numpy as np
import torch

from oracle import cpu_ref
from tests.helpers import default_dtype

EPS = 2.0 ** -24                 # half an fp32 ulp at 1: the unit of every bound
F32_TINY = 2.0 ** -126           # below fp32's normal range a rounding is absolute (2^-149), not relative
ACC_THRESHOLD = np.float32(1e-2)  # the reflect mask's accumulation threshold, as the reference model compares it (fp32)
CLIP_EXCLUDE = 1e-6              # a ray whose fp64 unclipped composite is this close to 0 or 1 may clip either way
CLIP_CAP = 0.02                  # ... at most this share of a case's rays
MASK_EXCLUDE = 1e-6              # a random ray whose fp64 |n.d| or |acc - 1e-2| is below this may fall on either side
MASK_CAP = 0.005
PLANTED = 5                      # composite_inputs plants rays 0 .. 4 (needs R >= 5)

COMPOSITE_S = (1, 63, 64, 65, 130, 192)   # one lane, a full wave +-1, three chunks with a ragged last one, the configs[3] size
COMPOSITE_R, COMPOSITE_LIVE = 37, 29
BIG_R, BIG_S = 32768 + 7, 5               # 8192 blocks x 4 rays = 32768: every wave walks a second ray, the last round is ragged
REFLECT_R = (1, 1023, 1024, 1025, 3001)
REFLECT_PATTERNS = ("none", "all", "random", "last")


def composite_seed(S, background):
    return 1000 + 10 * S + background


# ------------------------------------------------------------------------------------------------------------- compositing
def composite_inputs(R, S, seed):
    """fp32 inputs of one compositing case, after test_gpu_parity.test_composite: densities rand * 8 * (rand > 0.5), colours up to 2.0
    (a good share of rays leaves [0, 1]), jittered bins on [2, 6].  Upstream gradients are positive and unequal.  Planted rays:
      0  all sigma = 0;
      1  sigma = 1e4 in the first sample (plain bins: the first sample saturates);
      2  one zero-width bin with a finite sigma;
      3  colour == 1, sigma = 1e4 in sample 0, background row 1 (white): the composite is exactly 1.0 in fp32 and in fp64;
      4  colour == 0, background row 0: without a background (or with the per-ray one) the composite is exactly 0.0."""
    assert R >= PLANTED
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    sigma = rand(R, S) * 8.0 * (rand(R, S) > 0.5)
    nears, fars = torch.full((R, 1), 2.0), torch.full((R, 1), 6.0)
    _, eb = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, S, rand(R, S + 1))
    _, eb_plain = cpu_ref.spaced_bins("uniform", 1.0, nears, fars, S, None)
    eb = eb.clone()
    color = rand(R, S, 3) * 2.0
    inp = {"roughness": rand(R, S), "bg": rand(R, 3), "g_rgb": 0.25 + rand(R, 3), "g_rough": 0.25 + rand(R),
           "g_acc": 0.25 + rand(R), "normals": torch.nn.functional.normalize(torch.randn(R, S, 3, generator=g), dim=-1),
           "pred_normals": torch.nn.functional.normalize(torch.randn(R, S, 3, generator=g), dim=-1),
           "n_dot_d": rand(R, S) - 0.5}
    sigma[0] = 0.0
    sigma[1, 0], eb[1] = 1e4, eb_plain[1]
    j = S // 2
    eb[2, j + 1] = eb[2, j]
    sigma[2, j] = 3.0
    sigma[3, 0], eb[3], color[3], inp["bg"][3] = 1e4, eb_plain[3], 1.0, 1.0
    color[4], inp["bg"][4] = 0.0, 0.0
    inp.update(sigma=sigma, eb=eb.contiguous(), color=color)
    return inp


def _suffix_exclusive(x):
    """sum_{i>k} x_i along the last dimension, added from the far end (no subtraction of prefixes)."""
    s = torch.flip(torch.cumsum(torch.flip(x, [-1]), -1), [-1])
    return torch.cat([s[..., 1:], torch.zeros_like(s[..., :1])], -1)


def composite_reference(inp, background, detach_weights, clip, use_rough=True, use_g_rough=True, use_g_acc=True):
    """fp64 compositing forward and, by autograd, the gradients of
        loss = sum(g_rgb . rgb) + sum(g_rough . rendered roughness) + sum(g_acc . accumulation)
    through cpu_ref.weights_from_density / cpu_ref.composite_rgb (weights detached if detach_weights, torch.clip(rgb, 0, 1) before the
    loss if clip).  Also the per-output error scales: the sum of the absolute values of the terms each output adds.
      weights[k] = T_k - T_{k+1}                              scale T_k + T_{k+1}
      sums over the samples of w * v                          scale sum (T_k + T_{k+1}) |v|   (+ |bg| (1 + sum w) for the background)
      g_color, g_roughness_sample = w * g                     scale (T_k + T_{k+1}) |g|
      g_bg = g (1 - sum w)                                    scale |g| (1 + sum w)
      g_sigma[k] = delta_k (g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i)
                                                              scale delta_k (|g_w|[k] T_{k+1} + sum_{i>k} |g_w|[i] w_i), |g_w| = the sum of
        the absolute values of g_w's own terms g_c (colour_c - bg_c), g_rough roughness, g_acc (equal to |g_w[k]| wherever they share a
        sign: always without a background, the upstreams being positive), + 2^-29 delta_k sum_i |g_w|[i] w_i: the scans run in fp64, and
        one fp64 rounding (2^-53) of the ray's total is 2^-29 of it in units of 2^-24 -- what is left behind an opaque sample.
    Every scale also carries F32_TINY (fp32's denormal range).  `clip_near`: rays the clip-mask exclusion rule covers.
    -> (reference, scale, depth).  depth[name]: what fp32 itself does to exp(-X) -- X rounded to fp32 is off by up to X 2^-24, and so
    is exp(-X), relatively; for X in [32, 64) that alone is 32 x 2^-24, whatever the kernel does (the reference model's fp32 torch
    included).  With X_k = sum_{j<k} x_j:  w_k = (1 - exp(-x_k)) exp(-X_k) carries xw_k = w_k X_k + x_k T_{k+1}, T_{k+1} carries
    X_{k+1} T_{k+1}; depth[name] replaces every w / T of the scale by those.  A comparison allows 2^-24 depth on top of bound x scale:
    derived from the number format, not measured."""
    with default_dtype(torch.float64):
        R, S = inp["sigma"].shape
        leaf = lambda t: t.double().clone().requires_grad_(True)  # noqa: E731
        sigma, color, rough, bg = leaf(inp["sigma"]), leaf(inp["color"]), leaf(inp["roughness"]), leaf(inp["bg"])
        eb = inp["eb"].double()
        t0, t1 = eb[:, :-1], eb[:, 1:]
        g_rgb = inp["g_rgb"].double()
        g_r = inp["g_rough"].double() if (use_rough and use_g_rough) else torch.zeros(R)
        g_a = inp["g_acc"].double() if use_g_acc else torch.zeros(R)
        w = cpu_ref.weights_from_density(sigma[..., None], t0, t1)
        wl = w.detach() if detach_weights else w
        bgt = {0: None, 1: torch.ones(3), 2: bg}[background]
        unclipped = cpu_ref.composite_rgb(color, wl, bgt, True)
        rgb = torch.clip(unclipped, 0, 1) if clip else unclipped
        acc = wl.sum(dim=-2)[..., 0]
        rr = (wl[..., 0] * rough).sum(dim=-1)
        loss = (g_rgb * rgb).sum() + (g_r * rr).sum() + (g_a * acc).sum()
        loss.backward()
        grad = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
        ref = {"g_sigma": grad(sigma), "g_color": grad(color), "g_bg": grad(bg),
               "g_roughness_sample": grad(rough) if use_rough else None,
               "weights": w.detach()[..., 0], "rgb": rgb.detach(), "unclipped": unclipped.detach(), "accumulation": acc.detach(),
               "roughness": rr.detach()}
        # scales
        wd = ref["weights"]
        delta = t1 - t0
        x = delta * sigma.detach()
        T_next = torch.exp(-torch.cumsum(x, -1))
        T = torch.cat([torch.ones(R, 1), T_next[:, :-1]], -1)
        tt = T + T_next
        inside = (ref["unclipped"] >= 0) & (ref["unclipped"] <= 1)
        g_eff = g_rgb * inside if clip else g_rgb
        bgv = {0: torch.zeros(R, 3), 1: torch.ones(R, 3), 2: bg.detach()}[background]
        cd = color.detach()
        gw_terms = g_eff[:, None, :] * (cd - bgv[:, None, :])
        gw_abs = gw_terms.abs().sum(-1) + g_a[:, None].abs()
        gw = gw_terms.sum(-1) + g_a[:, None]
        if use_rough:
            gw_abs = gw_abs + (g_r[:, None] * rough.detach()).abs()
            gw = gw + g_r[:, None] * rough.detach()
        total_abs = (gw_abs * wd).sum(-1, keepdim=True)
        sc_sigma = delta * (gw_abs * T_next + _suffix_exclusive(gw_abs * wd) + 2.0 ** -29 * total_abs)
        sc_sigma_literal = delta * (gw.abs() * T_next + _suffix_exclusive(gw.abs() * wd))
        scale = {"g_sigma": sc_sigma, "g_sigma_literal": sc_sigma_literal,
                 "g_color": tt[..., None] * g_eff[:, None, :].abs().expand(R, S, 3),
                 "g_roughness_sample": tt * g_r[:, None].abs(),
                 "g_bg": g_eff.abs() * (1 + ref["accumulation"])[:, None],
                 "weights": tt,
                 "rgb": (tt[..., None] * cd.abs()).sum(-2) + bgv.abs() * (1 + ref["accumulation"])[:, None] * (background != 0),
                 "accumulation": tt.sum(-1),
                 "roughness": (tt * rough.detach()).sum(-1)}
        scale = {k: v + F32_TINY for k, v in scale.items()}
        X_next = torch.cumsum(x, -1)
        X = torch.cat([torch.zeros(R, 1), X_next[:, :-1]], -1)
        xw = wd * X + x * T_next
        depth = {"g_sigma": delta * (gw_abs * T_next * X_next + _suffix_exclusive(gw_abs * xw)),
                 "g_color": xw[..., None] * g_eff[:, None, :].abs().expand(R, S, 3),
                 "g_roughness_sample": xw * g_r[:, None].abs(),
                 "g_bg": g_eff.abs() * xw.sum(-1)[:, None],
                 "weights": xw,
                 "rgb": (xw[..., None] * cd.abs()).sum(-2) + bgv.abs() * xw.sum(-1)[:, None] * (background != 0),
                 "accumulation": xw.sum(-1),
                 "roughness": (xw * rough.detach()).sum(-1)}
        if detach_weights:
            scale["g_sigma"] = torch.zeros(R, S)  # exactly zero
        u = ref["unclipped"]
        # exactly on a bound is not "near": that takes exact zeros (sigma == 0 gives w == 0) or the planted saturation, which fp32
        # reproduces bit for bit, and torch.clamp passes the gradient there
        near = ((((u - 0).abs() < CLIP_EXCLUDE) & (u != 0)) | (((u - 1).abs() < CLIP_EXCLUDE) & (u != 1))).any(-1)
        near[:PLANTED] = False  # the planted rays are never left out
        ref["clip_near"] = near if clip else torch.zeros(R, dtype=torch.bool)
        ref["gw"] = gw
        ref["T_next"] = T_next
    return ref, scale, depth


def composite_closed_form(inp, background, clip):
    """g_sigma of the same loss from the closed form in rsn_render.hip's header comment, coded on its own in fp64:
        dL/dx_k = g_w[k] T_{k+1} - sum_{i>k} g_w[i] w_i,  g_sigma[k] = delta_k dL/dx_k,
    with w_i = (1 - exp(-x_i)) T_i, T_i = exp(-sum_{j<i} x_j) built by a plain loop over the samples."""
    with default_dtype(torch.float64):
        sigma, eb, color = inp["sigma"].double(), inp["eb"].double(), inp["color"].double()
        R, S = sigma.shape
        bg = {0: torch.zeros(R, 3), 1: torch.ones(R, 3), 2: inp["bg"].double()}[background]
        delta = eb[:, 1:] - eb[:, :-1]
        x = delta * sigma
        T = torch.ones(R, S + 1)
        for k in range(S):
            T[:, k + 1] = T[:, k] * torch.exp(-x[:, k])
        w = (1 - torch.exp(-x)) * T[:, :S]
        acc = w.sum(-1)
        comp = (w[..., None] * color).sum(1) + bg * (1 - acc)[:, None]
        g = inp["g_rgb"].double()
        if clip:
            g = g * ((comp >= 0) & (comp <= 1))
        gw = (g[:, None, :] * (color - bg[:, None, :])).sum(-1) + inp["g_rough"].double()[:, None] * inp["roughness"].double() \
            + inp["g_acc"].double()[:, None]
        out = torch.zeros(R, S)
        for k in range(S):
            out[:, k] = delta[:, k] * (gw[:, k] * T[:, k + 1] - (gw[:, k + 1:] * w[:, k + 1:]).sum(-1))
    return out


def ray_losses_reference(inp, weights64):
    """pn_loss_ray = sum_s w |n - pn|^2, ori_loss_ray = sum_s w max(0, n.d)^2 in fp64, with their scales (weights scale: see
    composite_reference)."""
    with default_dtype(torch.float64):
        e2 = ((inp["normals"].double() - inp["pred_normals"].double()) ** 2).sum(-1)
        nd2 = inp["n_dot_d"].double().clamp(min=0) ** 2
        return (weights64 * e2).sum(-1), (weights64 * nd2).sum(-1), e2, nd2


# ------------------------------------------------------------------------------------------------------------- reflect setup
def reflect_seed(R, pattern):
    return 5000 + 7 * R + REFLECT_PATTERNS.index(pattern)


def reflect_inputs(R, pattern, seed):
    """fp32 inputs of rsn_reflect_setup.  So that the relative bounds of the fixed short chains hold against fp64, nothing here
    cancels: the three products of n.d share a sign (n = s * sign(d) * |.|, s = -1 for a ray facing the camera), and so do
    origins and depth * directions.  pattern: which rays (acc > 1e-2) & (n.d < 0) selects --
      none    no ray (accumulations below the threshold);
      all     every ray;
      random  about 40 %;
      last    rays of the last 1024-ray block only.
    random with R >= 8, and last with as many rays in its last block, also carry the planted threshold rays (the last four):
      R-1  acc == float32(1e-2), n.d < 0: not masked;      R-2  acc == nextafter(float32(1e-2), 1): masked;
      R-3  n.d == 0 exactly (axis-aligned vectors): not masked;  R-4  n.d == -2^-20: masked.
    -> (inputs, planted ray indices)."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    facing = {"none": torch.ones(R, dtype=torch.bool), "all": torch.ones(R, dtype=torch.bool),
              "random": rand(R) < 0.64, "last": rand(R) < 0.64}[pattern]
    sgn = torch.where(d >= 0, torch.ones(()), -torch.ones(()))
    n = torch.nn.functional.normalize(torch.randn(R, 3, generator=g).abs() + 0.05, dim=-1) * sgn
    n = torch.where(facing[:, None], -n, n)
    acc = rand(R) * 0.009 if pattern == "none" else 0.02 + 0.98 * rand(R)
    if pattern in ("random", "last"):
        low = rand(R) < 0.375  # 0.64 * 0.625 = 0.4
        acc = torch.where(low, rand(R) * 0.009, acc)
    if pattern == "last":
        first = ((R - 1) // 1024) * 1024
        acc[:first] = rand(first) * 0.009
    inp = {"origins": sgn * (0.5 + rand(R, 3)), "directions": d, "accumulation": acc, "depth": 2.0 + 4.0 * rand(R),
           "pred_normals": n, "roughness": 0.05 + 0.9 * rand(R)}
    planted = []
    if pattern == "random" and R >= 8 or pattern == "last" and R - ((R - 1) // 1024) * 1024 >= 8:  # inside the last block
        thr = ACC_THRESHOLD
        acc[R - 1] = float(thr)
        acc[R - 2] = float(np.nextafter(thr, np.float32(1.0)))
        for r in (R - 1, R - 2):  # decisive n.d < 0
            inp["pred_normals"][r] = -inp["pred_normals"][r].abs() * sgn[r]
        ax = torch.tensor([1.0, 0.0, 0.0])
        for r in (R - 3, R - 4):
            d[r], acc[r] = ax, 0.5
            inp["origins"][r] = torch.tensor([1.0, 1.0, 1.0])
        inp["pred_normals"][R - 3] = torch.tensor([0.0, 1.0, 0.0])
        inp["pred_normals"][R - 4] = torch.tensor([-2.0 ** -20, 1.0, 0.0])
        planted = [R - 1, R - 2, R - 3, R - 4]
    return inp, planted


def reflect_reference(inp, planted, reflect_far):
    """fp64 restatement of rsn_reflect_setup (include/rsn.h; reference model.py:222-229, 240-241, 267-289).  The mask thresholds are
    compared as the reference model compares them: the fp32 accumulation against np.float32(1e-2), n.d against 0.
    -> (reference, near: random rays within MASK_EXCLUDE of a threshold, which may fall on either side)."""
    with default_dtype(torch.float64):
        o, d, n = inp["origins"].double(), inp["directions"].double(), inp["pred_normals"].double()
        ndd = (n * d).sum(-1)
        acc32 = inp["accumulation"].numpy()
        mask = torch.from_numpy(acc32 > ACC_THRESHOLD) & (ndd < 0)
        near = (ndd.abs() < MASK_EXCLUDE) | ((inp["accumulation"].double() - float(ACC_THRESHOLD)).abs() < MASK_EXCLUDE)
        if planted:
            near[planted] = False
        rf = d - 2 * ndd[:, None] * n
        rough = inp["roughness"].double()
        sq = 2 * ndd.abs() * rough ** 2
        ref = {"mask": mask, "n_dot_d": ndd, "origins2": o + inp["depth"].double()[:, None] * d,
               "directions2": rf / rf.norm(dim=-1, keepdim=True).clamp(min=1e-12), "sqradius": sq, "pixel_area2": np.pi * sq,
               "nears2": torch.zeros_like(sq), "fars2": torch.full_like(sq, float(np.float32(reflect_far))),
               "reflect_default": (torch.ones((), dtype=torch.float32) - inp["accumulation"])}  # one IEEE fp32 subtraction: exact
    return ref, near


def combine_inputs(R, seed, ray_index):
    """diff, tint, g_out [R,3] by original ray and a composite comp [R,3] by compacted ray (row i belongs to ray ray_index[i]; rows
    behind M are filler) for rsn_reflect_combine: v = diff + tint * comp covers (-inf, 0), (0, 1) and (1, inf) decisively without
    cancellation (diff and comp share a sign per element, tint > 0), plus planted elements on the first two reflected rays where v is
    exactly 1, 0, 0 (0.25 + 0.5 * 1.5; 0 + 0.5 * 0; -0.75 + 0.5 * 1.5) and 1, 1, 1 in fp32 and in fp64."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    s = torch.where(rand(R, 3) < 0.25, -torch.ones(()), torch.ones(()))
    diff, tint, comp_by_ray = s * 0.6 * rand(R, 3), 0.05 + 0.95 * rand(R, 3), s * 2.0 * rand(R, 3)
    exact = torch.zeros(R, dtype=torch.bool)
    M = ray_index.numel()
    if M >= 2:
        a, b = int(ray_index[0]), int(ray_index[1])
        diff[a], tint[a], comp_by_ray[a] = torch.tensor([0.25, 0.0, -0.75]), torch.tensor([0.5, 0.5, 0.5]), torch.tensor([1.5, 0.0, 1.5])
        diff[b], tint[b], comp_by_ray[b] = torch.tensor([0.25, 0.25, 0.25]), torch.tensor([0.5, 0.5, 0.5]), torch.tensor([1.5, 1.5, 1.5])
        exact[a] = exact[b] = True
    comp = rand(R, 3)
    comp[:M] = comp_by_ray[ray_index]
    return {"diff": diff, "tint": tint, "comp": comp, "g_out": 0.25 + rand(R, 3), "exact": exact,
            "g_sqradius": 0.25 + rand(R), "g_pixel_area": 0.25 + rand(R), "g_coarse": 0.25 + rand(R, 3),
            "g_fine": 0.25 + rand(R, 3)}


def combine_reference(ci, ray_index):
    """ray_index: int64 [M], compacted ray i -> original ray; comp / g_out rows: comp by compacted ray, diff / tint / g_out by original
    ray (include/rsn.h).  -> v (unclipped), out = clip(v, 0, 1), g_comp = g_out * tint where 0 <= v <= 1, near (clip exclusion)."""
    with default_dtype(torch.float64):
        M = ray_index.numel()
        diff, tint = ci["diff"].double()[ray_index], ci["tint"].double()[ray_index]
        comp = ci["comp"].double()[:M]
        v = diff + tint * comp
        inside = (v >= 0) & (v <= 1)
        g_comp = torch.where(inside, ci["g_out"].double()[ray_index] * tint, torch.zeros(()))
        near = ((((v - 0).abs() < CLIP_EXCLUDE) & (v != 0)) | (((v - 1).abs() < CLIP_EXCLUDE) & (v != 1))).any(-1) \
            & ~ci["exact"][ray_index]
    return {"v": v, "out": v.clamp(0, 1), "g_comp": g_comp, "near": near}


# ------------------------------------------------------------------------------------------------------------- losses
LOSS_R = (1, 341, 342, 1024, 4099)
LOSS_COEF = (1.0, 0.5, 0.25, 2.0, 3e-4, 1e-3, 1e-2, 1e-1)
LOSS_UPSTREAM = (1.0, 0.75, 1.5, 2.0, 0.5, 3.0, 1.25, 0.125)


def loss_rays_inputs(R, seed):
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    return {"image": rand(R, 3), "rgb4": [rand(R, 3) for _ in range(4)], "pn_ray2": [rand(R) for _ in range(2)],
            "ori_ray2": [rand(R) * 0.1 for _ in range(2)]}


def loss_rays_reference(li, coef):
    """The eight unscaled terms and g_rgb4[k] = coef[k] * 2 (rgb - image) / (3 R) in fp64 (include/rsn.h).  All terms of every sum
    are positive: a sum is its own scale."""
    with default_dtype(torch.float64):
        img = li["image"].double()
        n3 = img.numel()
        c = [float(np.float32(v)) for v in coef]
        losses = [((r.double() - img) ** 2).sum() / n3 for r in li["rgb4"]]
        losses += [p.double().sum() for p in li["pn_ray2"]] + [p.double().sum() for p in li["ori_ray2"]]
        g = [c[k] * 2 * (li["rgb4"][k].double() - img) / n3 for k in range(4)]
    return torch.stack(losses), g
