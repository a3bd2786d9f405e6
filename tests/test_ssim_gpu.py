"""rsn_ssim (csrc/rsn_data.hip) against the float64 map of tests/ssim_reference.py: every case of its table -- window grids that end on,
before and after the 32 x 16 tile seams, one with more than 256 workgroups; rendered-like, constant-target, 0/1, single-pixel,
per-channel, scaled and explicit-range images -- within the case's derived bound (4x the float32 restatement's error + 2^-24; nothing
measured on the kernel), then scaling by powers of two, an explicit data range, symmetry and repeatability bit for bit from poisoned
buffers, and the workspace contract.  tests/test_ssim_cpu.py shows that these cases can fail."""
import contextlib

import numpy as np
import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, metrics
from tests import ssim_reference as R
from tests.helpers import _POISON, _poisoned

pytestmark = pytest.mark.gpu

SEAM_PAIRS = ("random", "render_like")  # x the shape with one full tile plus a single row and column
_dead = []


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


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


def _on(dev, *arrays):
    return [torch.from_numpy(a.copy()).to(dev) for a in arrays]  # the cases are read-only: copy


def _buffers(dev, H, W, short=0):
    """Poisoned workspace (the fp64 partials, as NaN words) of rsn_ssim_workspace_bytes less `short` bytes, and a poisoned output."""
    need = int(pkg.load_library().rsn_ssim_workspace_bytes(H, W))
    assert need == 8 * int(np.prod(R.grid(H, W)))
    b = _poisoned({"ws": torch.empty(need // 4, dtype=torch.float32, device=dev), "out": torch.empty(1, dtype=torch.float32, device=dev)})
    return b["ws"], need - short, b["out"]


def _direct(dev, p, t, data_range):
    """rsn_ssim through the C ABI with the caller's data range in a one-element device tensor -> the 0-d result (poisoned before)."""
    H, W = int(p.shape[0]), int(p.shape[1])
    L = torch.tensor([data_range], dtype=torch.float32, device=dev)
    ws, nbytes, out = _buffers(dev, H, W)
    _abi.check(pkg.load_library().rsn_ssim(H, W, _abi.ptr(p), _abi.ptr(t), _abi.ptr(L), _abi.ptr(ws), nbytes, _abi.ptr(out),
                                           torch.cuda.current_stream(dev).cuda_stream))
    return out[0]


def measure(dev, name):
    """One case on the device -> (the kernel's value, its reference row)."""
    p, t, L = R.case(name)
    a, b = _on(dev, p, t)
    with _launching():
        got = metrics.ssim(a, b) if L is None else _direct(dev, a, b, L)
        assert got.dim() == 0 and got.device.type == "cuda" and got.dtype == torch.float32
        got = float(got)
    return got, R.reference(name)


@pytest.mark.parametrize("cls", R.CLASSES)
def test_every_case_within_its_bound_of_float64(dev, cls):
    """|rsn_ssim - ssim_mean(float64)| <= 4 |ssim_mean(float32) - ssim_mean(float64)| + 2^-24 per case.  For the impulse cases the
    figures also read as window positions: (1 - mean) x count is the sum of what the 121 x 3 terms around the pixel lack of 1."""
    failed = []
    for name in R.names(cls):
        got, r = measure(dev, name)
        err = abs(got - r["ref"])
        line = f"{name}: got {got:.9f} ref {r['ref']:.9f} err {err:.3e} float32 {r['f32_err']:.3e} bound {r['bound']:.3e} ({err / r['bound']:.2f})"
        if cls == "impulse":
            line += f"; (1 - mean) x count: got {(1.0 - got) * r['count']:.5f}, ref {(1.0 - r['ref']) * r['count']:.5f}"
        print(line)
        if not err <= r["bound"]:
            failed.append(line)
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("base", SEAM_PAIRS)
def test_power_of_two_scaling_is_exact(dev, base):
    """ssim(k a, k b) == ssim(a, b) bit for bit for k = 4, 1/4: the data range comes through the pointer, every product, c1 and c2
    scale by a power of two, and nothing comes near the denormal range.  A kernel that took L = 1 fails this."""
    p, t, _ = R.case(f"{base}_{R._tag(R.TWO_TILES)}")
    a, b = _on(dev, p, t)
    with _launching():
        want = metrics.ssim(a, b)
        for k in R.SCALES:
            assert torch.equal(metrics.ssim(a * k, b * k), want), (base, k)


def test_explicit_data_range_differs_from_the_images_own(dev):
    """The C entry point with data_range = 1.0 on images whose own range is 0.5: within the bound of ssim_mean(float64, 1.0), and
    not the value the images' own range gives."""
    for name in R.names("explicit"):
        p, t, L = R.case(name)
        assert L == 1.0 and R.data_range_of(p, t) == 0.5
        a, b = _on(dev, p, t)
        with _launching():
            got, own = float(_direct(dev, a, b, L)), float(metrics.ssim(a, b))
        r = R.reference(name)
        own_ref = R.ssim_mean(p, t, None)
        print(f"{name}: range 1.0: got {got:.9f} ref {r['ref']:.9f} bound {r['bound']:.3e}; own range: got {own:.9f} ref {own_ref:.9f}")
        assert abs(got - r["ref"]) <= r["bound"]
        assert abs(own - own_ref) <= R.bound(R.ssim_mean(p, t, None, np.float32), own_ref)
        assert abs(own_ref - r["ref"]) > 100 * r["bound"]  # the two ranges are far apart on this pair


@pytest.mark.parametrize("shape", (R.TWO_TILES, R.THREE_TILES), ids=R._tag)
@pytest.mark.parametrize("base", SEAM_PAIRS + ("white_target", "channels"))
def test_symmetric_and_repeatable_from_poisoned_buffers(dev, base, shape):
    """ssim(a, b) has the bits of ssim(b, a) and of three repeats; workspace and output start as NaN words every time."""
    p, t, _ = R.case(f"{base}_{R._tag(shape)}")
    a, b = _on(dev, p, t)
    L = float(R.data_range_of(p, t))
    with _launching():
        ab, ba = _direct(dev, a, b, L), _direct(dev, b, a, L)
        again = [_direct(dev, a, b, L) for _ in range(3)]
        via_metrics = metrics.ssim(a, b)
    assert bool(torch.isfinite(ab)) and torch.equal(ab, ba)
    assert all(torch.equal(x, ab) for x in again)
    assert torch.equal(via_metrics, ab)  # metrics.ssim passes the same range, computed on the device


def test_workspace_size_is_exact(dev):
    """rsn_ssim_workspace_bytes is one fp64 per workgroup and is accepted at exactly that size for every shape of the table; one byte
    less is refused with RSN_ERR_WORKSPACE before anything is launched (the poisoned output and workspace stay as they were).
    tests/test_abi_cpu.py does not hold this."""
    lib = pkg.load_library()
    stream = torch.cuda.current_stream(dev).cuda_stream
    it, pattern = _POISON[torch.float32]
    for shape in R.SEAM_SHAPES + (R.BIG,):
        H, W = shape[0] + R.HALO, shape[1] + R.HALO
        p, t, _ = R.case(f"random_{R._tag(shape)}")
        a, b = _on(dev, p, t)
        L = torch.tensor([1.0], dtype=torch.float32, device=dev)
        ws, nbytes, out = _buffers(dev, H, W, short=1)
        rc = lib.rsn_ssim(H, W, _abi.ptr(a), _abi.ptr(b), _abi.ptr(L), _abi.ptr(ws), nbytes, _abi.ptr(out), stream)
        assert rc == -4 and b"workspace" in lib.rsn_last_error(), (shape, rc)  # RSN_ERR_WORKSPACE
        with pytest.raises(pkg.RsnError, match=f"{nbytes + 1} needed"):
            _abi.check(rc)
        with _launching():
            assert bool((out.view(it) == pattern).all()) and bool((ws.view(it) == pattern).all()), shape
            ws, nbytes, out = _buffers(dev, H, W)
            _abi.check(lib.rsn_ssim(H, W, _abi.ptr(a), _abi.ptr(b), _abi.ptr(L), _abi.ptr(ws), nbytes, _abi.ptr(out), stream))
            assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ws.view(torch.float64)).all()), shape
