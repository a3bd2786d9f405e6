"""The standalone encoders rsn_ipe_encode and rsn_sh34_encode (csrc/rsn_render.hip: rsn_ipe_kernel, rsn_sh34_kernel -- their own code,
beside the fused encoders that tests/test_field_maths_gpu.py covers), called through the C ABI on the contracted means, variances and
directions of field_maths_reference.build_inputs(): 2,680 points of every input class (pixel areas over nine decades, bins at 0,
of zero width, at 250 and out to 1e3, means either side of the contraction's branch, the SH poles, directions of length 1/2 and 2),
11 workgroups of the SH kernel with the last one partial; n = 1 and n = 0 beside them.

References: field_maths_reference.ipe_rows in float64 and float32 (the float32 phases taken as exact numbers, as everywhere), in the
reference's column order [sin 48 | cos 48 | raw 3], the raw columns bit-exact.  rsn_sh34_encode takes the attenuation exponent rho
itself (exp(-rho l (l + 1) / 2): IntegratedSHEncoding.forward's `roughness` argument), not the raw head value that sh_rows'
options start from, so its reference is restated here: cpu_ref.integrated_sh in float64 on the direction and the float32 rho the
kernel is handed, rho = softplus(raw roughness).  build_inputs() carries no raw roughness of its own (in the field tests it comes out
of the roughness head), so this file draws one per point, spread evenly over field_maths_reference.ROUGHNESS_SPAN and shuffled.
The rule is field_maths_reference.compare per input class (factor 4 over the float32 oracle's own error, plus its floor); nothing is
measured on the kernels.  Outputs are 64 rows longer than n and poisoned first; rows behind n keep the poison."""
import contextlib
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from oracle import cpu_ref
from reflect_sampling_nerf_amd import _abi, ops
from reflect_sampling_nerf_amd._abi import ptr
from tests import field_maths_reference as R
from tests.helpers import _check_count, _poisoned, default_dtype

pytestmark = pytest.mark.gpu
f32, f64 = torch.float32, torch.float64
TAIL = 64


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


_INPUTS = {}


def inputs():
    """The points once per run: float32 means / variances / directions / rho as the kernels read them, and the class of each point."""
    if not _INPUTS:
        inp = R.build_inputs()
        mean, var, _ = R.gaussian(inp, f64)
        N = mean.shape[0]
        assert N == 2680 and -(-N // 256) == 11 and N % 256
        raw = torch.linspace(R.ROUGHNESS_SPAN[0], R.ROUGHNESS_SPAN[1], N, dtype=f64)[torch.randperm(N, generator=torch.Generator().manual_seed(6))]
        _INPUTS.update({"mean": mean.float().contiguous(), "var": var.float().contiguous(), "dirs": R.point_dirs(inp, f32).contiguous(),
                        "rho": torch.nn.functional.softplus(raw).float().contiguous(), "cls": R.point_class(inp), "names": inp["names"],
                        "freqs": R.frequencies()})
    return _INPUTS


def sh_reference(dirs32, rho32, dtype):
    with default_dtype(dtype):
        return cpu_ref.integrated_sh(dirs32.to(dtype), rho32.to(dtype).reshape(-1, 1))


def _among_all(got, ref):
    """The n rows a launch wrote among all 2,680 (the others exact): a launch of one point is held to the bound of its class, the
    oracle's worst error over the class, not to the oracle's luck on that point."""
    full = ref.double().clone()
    full[: got.shape[0]] = got.double()
    return full


def _finish(v):
    print(v.report())
    assert v.ok, "\n" + v.report()


def _ipe(dev, n, with_cov):
    lib = _abi.load_library()
    d = inputs()
    out = _poisoned({"out": torch.empty(n + TAIL, 99, device=dev)})
    mean, var = d["mean"][:max(n, 1)].to(dev), d["var"][:max(n, 1)].to(dev)
    freqs = (C.c_float * 16)(*[float(x) for x in d["freqs"]])
    with _launching():
        _abi.check(lib.rsn_ipe_encode(n, ptr(mean), ptr(var) if with_cov else None, freqs, ptr(out["out"]), ops._stream()))
    _check_count(f"ipe n{n}", out, n)
    return out["out"][:n].cpu()


@pytest.mark.parametrize("with_cov", [True, False], ids=["cov_diag", "no_cov"])
@pytest.mark.parametrize("n", [2680, 1, 0])
def test_ipe_encode_against_fp64(dev, n, with_cov):
    d = inputs()
    got = _ipe(dev, n, with_cov)
    if n == 0:
        return
    mean, var = d["mean"], d["var"] if with_cov else torch.zeros_like(d["var"])
    assert torch.equal(got[:, 96:].view(torch.int32), mean[:n].view(torch.int32)), "the raw columns are the input's bits"
    ref, ora = (R.ipe_rows(mean, var, d["freqs"], dt) for dt in (f64, f32))
    _finish(R.compare(f"ipe n{n}{'' if with_cov else ' no cov'}", "ipe_encode", _among_all(got[:, :96], ref), ref, ora, d["cls"], d["names"]))


def _sh(dev, n, with_rho):
    lib = _abi.load_library()
    d = inputs()
    out = _poisoned({"out": torch.empty(n + TAIL, 34, device=dev)})
    dirs, rho = d["dirs"][:max(n, 1)].to(dev), d["rho"][:max(n, 1)].to(dev)
    with _launching():
        _abi.check(lib.rsn_sh34_encode(n, ptr(dirs), ptr(rho) if with_rho else None, ptr(out["out"]), ops._stream()))
    _check_count(f"sh34 n{n}", out, n)
    return out["out"][:n].cpu()


@pytest.mark.parametrize("with_rho", [True, False], ids=["roughness", "no_roughness"])
@pytest.mark.parametrize("n", [2680, 1, 0])
def test_sh34_encode_against_fp64(dev, n, with_rho):
    d = inputs()
    got = _sh(dev, n, with_rho)
    if n == 0:
        return
    dirs, rho = d["dirs"], d["rho"] if with_rho else torch.zeros_like(d["rho"])
    ref, ora = (sh_reference(dirs, rho, dt) for dt in (f64, f32))
    _finish(R.compare(f"sh34 n{n}{'' if with_rho else ' no roughness'}", "sh34_encode", _among_all(got, ref), ref, ora, d["cls"], d["names"]))
