"""fp64 reference, inputs and the comparison rule for one step of rsn_radam_step (csrc/rsn_train_ops.hip), from explicit state:
parameters p, moments m and v in float32, the step number t.  One step at a time, so that an error can neither build up nor cancel
across steps.  The reference is torch.optim.RAdam on float64 copies of the same bits, brought to step t - 1 through load_state_dict;
the same in float32 is the oracle whose own error sets the bound (field_maths_reference.compare, mode "scaled", factor 4), per
gradient decade.  Nothing here is measured on the kernel.

Scales, per element, from the fp64 values:   p: |p| + |update|     m: |beta1 m| + |(1 - beta1) g|     v: |beta2 v| + |(1 - beta2) g^2|

The hyper-parameters cross the C ABI as float.  The reference takes the values the kernel receives (BETAS, LRS, EPSS are float32
numbers written as Python floats): the check is of the step's arithmetic, not of how 0.999 rounds to float32.  Likewise the inputs
keep (1 - beta2) g^2 above float32's smallest normal number (|g| >= 1e-12): denormal handling is not what is checked.

Users: tests/test_radam_cpu.py (the rule against a float32 emulation and its planted faults), tests/test_radam_gpu.py."""
import math

import numpy as np
import torch

from tests import field_maths_reference as FM

f32, f64 = torch.float32, torch.float64
_r = lambda x: float(np.float32(x))  # noqa: E731
BETAS = (_r(0.9), _r(0.999))
LRS = (_r(1e-3), _r(1e-6))
EPSS = (_r(1e-15), _r(1e-8))
STEPS = (1, 5, 6, 7, 1000, 50000)
G_DECADES = tuple(range(-12, 3))  # |g| log-uniform over 1e-12 .. 1e3
NAMES = [f"g_1e{d}" for d in G_DECADES] + ["g_zero"]
SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 90880)  # 256 x 256 threads: 65,537 is the first size the stride loop serves


def rho(t, beta2=BETAS[1]):
    """rho_t of the RAdam paper in fp64; the update is rectified where rho_t > 5."""
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    bt = beta2 ** t
    return rho_inf - 2.0 * t * bt / (1.0 - bt)


def switch_steps(steps=STEPS):
    """-> (steps with rho_t <= 5, steps with rho_t > 5); asserts that the list holds the two steps either side of the switch."""
    below, above = [t for t in steps if rho(t) <= 5.0], [t for t in steps if rho(t) > 5.0]
    assert below and above and max(below) + 1 == min(above), (below, above)
    return below, above


_STATES = {}


def make_state(n, seed, fresh=False):
    """p, g, m, v [n] float32 and the class of each element.  |g| log-uniform over 1e-12 .. 1e3 with both signs, one element in
    sixteen an exact zero; m and v as a previous step left them (of a gradient within a decade of g, either sign), or zeros
    (fresh); half of the g == 0 elements have m == v == 0; p half of order 1, half log-uniform over 1e-8 .. 1e-2, a few exact zeros.
    The previous gradient is a factor 2 to 10 above or below |g|, so that beta1 m + (1 - beta1) g of opposite signs keeps at least
    a quarter of its larger term: the error of the update relative to the update grows with that cancellation, and the scale the
    rule gives p, |p| + |update|, has no term for it (at |previous g| = 1.11 |g| the new m cancels altogether)."""
    key = (n, seed, fresh)
    if key in _STATES:
        return _STATES[key]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.rand(n, generator=gen, dtype=f64)  # noqa: E731
    sign = lambda: torch.where(rnd() < 0.5, -1.0, 1.0).to(f64)  # noqa: E731
    mag = 10.0 ** (-12.0 + 15.0 * rnd())
    g = sign() * mag
    zero = rnd() < 1.0 / 16
    g[zero] = 0.0
    g_prev = sign() * mag * 10.0 ** (sign() * (0.3 + 0.7 * rnd()))  # a factor 2 .. 10 either way: see the docstring
    m, v = (1.0 - BETAS[0]) * g_prev, (1.0 - BETAS[1]) * g_prev * g_prev
    blank = zero & (rnd() < 0.5)
    m[blank], v[blank] = 0.0, 0.0
    if fresh:
        m, v = torch.zeros(n, dtype=f64), torch.zeros(n, dtype=f64)
    p = torch.where(rnd() < 0.5, torch.randn(n, generator=gen, dtype=f64), sign() * 10.0 ** (-8.0 + 6.0 * rnd()))
    p[rnd() < 1.0 / 64] = 0.0
    g32 = g.float()
    cls = torch.where(g32 == 0, torch.tensor(len(G_DECADES)), (torch.floor(torch.log10(g32.double().abs().clamp_min(1e-300))).long() + 12).clamp(0, len(G_DECADES) - 1))
    st = {"n": n, "p": p.float(), "g": g32, "m": m.float(), "v": v.float(), "cls": cls, "key": key}
    nz = st["g"][st["g"] != 0].double()
    assert nz.numel() == 0 or float(((1.0 - BETAS[1]) * nz * nz).min()) > 1.2e-38
    _STATES[key] = st
    return st


def torch_step(st, t, lr, eps, dtype, coef=None):
    """One torch.optim.RAdam step number t in `dtype` from the state's bits -> (p, m, v).  coef: the factor a clipped step reads the
    gradients with (float32, as the guarded kernel recorded it)."""
    p = torch.nn.Parameter(st["p"].to(dtype).clone())
    opt = torch.optim.RAdam([p], lr=lr, betas=BETAS, eps=eps, foreach=False)
    sd = opt.state_dict()
    sd["state"] = {0: {"step": torch.tensor(float(t - 1)), "exp_avg": st["m"].to(dtype).clone(), "exp_avg_sq": st["v"].to(dtype).clone()}}
    opt.load_state_dict(sd)
    g = st["g"].to(dtype)
    p.grad = g if coef is None else g * torch.tensor(coef, dtype=dtype)
    opt.step()
    s = opt.state[p]
    assert int(s["step"]) == t and s["exp_avg"].dtype == dtype
    return p.detach(), s["exp_avg"], s["exp_avg_sq"]


_REFS = {}


def references(st, t, lr, eps, coef=None):
    """-> {"ref": (p, m, v) in fp64, "oracle": the same in float32, "scale": (s_p, s_m, s_v)}, computed once per (state, t, lr, eps, coef)."""
    key = (st["key"], t, lr, eps, coef)
    if key not in _REFS:
        ref, ora = torch_step(st, t, lr, eps, f64, coef), torch_step(st, t, lr, eps, f32, coef)
        p0, m0, v0 = st["p"].double(), st["m"].double(), st["v"].double()
        g = st["g"].double() * (1.0 if coef is None else coef)
        scale = (p0.abs() + (ref[0] - p0).abs(), (BETAS[0] * m0).abs() + ((1.0 - BETAS[0]) * g).abs(),
                 (BETAS[1] * v0).abs() + ((1.0 - BETAS[1]) * g * g).abs())
        if len(_REFS) > 64:
            _REFS.clear()
        _REFS[key] = {"ref": ref, "oracle": ora, "scale": scale}
    return _REFS[key]


def slice_state(st, a, b):
    """Elements [a, b) of a state as a tensor of their own (the launch's view of it); judged as part of `st` by judge_pieces."""
    return {"n": b - a, "offset": a, **{k: st[k][a:b] for k in ("p", "g", "m", "v")}}


def judge_pieces(label, st, t, lr, eps, pieces, coef=None):
    """pieces: [(offset, (p, m, v))] -- the elements of `st` that a launch updated, as host tensors.  The oracle's worst error of a
    class is taken over the whole state, so that a tensor of one element is held to the bound of its class, not to the luck of the
    oracle on that one element; elements outside the pieces count as exact.  -> [Verdict of p, of m, of v]."""
    r = references(st, t, lr, eps, coef)
    vs = []
    for k, q in enumerate(("radam p", "radam m", "radam v")):
        got = r["ref"][k].double().clone()
        for off, outs in pieces:
            got[off: off + outs[k].numel()] = outs[k].double()
        vs.append(FM.compare(label, q, got.reshape(-1, 1), r["ref"][k].reshape(-1, 1), r["oracle"][k].reshape(-1, 1), st["cls"], NAMES,
                             mode="scaled", scale=r["scale"][k]))
    return vs


def judge(label, st, t, lr, eps, p, m, v, coef=None):
    """The whole state after the step under test (host tensors [n]) -> [Verdict of p, of m, of v]."""
    return judge_pieces(label, st, t, lr, eps, [(0, (p, m, v))], coef)


def report(vs):
    return "\n".join(v.report() for v in vs)


def worst_share(vs):
    return max((r["got"] / r["bound"] for v in vs for r in v.rows), default=0.0)


assert math.isclose(BETAS[1], 0.999, rel_tol=1e-7)
