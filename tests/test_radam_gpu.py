"""rsn_radam_step (csrc/rsn_train_ops.hip) one step at a time through the C ABI, against torch.optim.RAdam in float64 from the same
explicit state (tests/optimizer_reference.py): both branches of the rectification and the two steps either side of the switch, two
learning rates and two eps, gradients over fifteen decades with exact zeros, moments of a previous step and fresh ones; tensor
sizes either side of a block (256) and of the grid's cap (256 blocks: 65,537 elements is the first size the stride loop serves);
48 tensors in one launch, the limit, with an empty tensor and tensors without a gradient; the refusals at 49 tensors and at step 0.
The guarded path (rsn_grad_sumsq + rsn_radam_step_guarded through FusedRAdam) is held to the unguarded launch bit for bit where it
does not clip, and to the same rule with g * coef where it does.

The rule is field_maths_reference.compare in mode "scaled", factor 4 over torch's own float32 step, per gradient decade; no bound is
a number taken from the kernel.  tests/test_radam_cpu.py shows the rule passing a float32 emulation and rejecting its planted
faults, the rectification factor off by 1e-3 among them.  Every check prints its verdict (tools/step_edges_report.py collects them
into profiles/step_edges.json).

Every buffer is 64 elements longer than its tensor and filled with tests.helpers._POISON first; the tails must keep it.
FusedRAdam hands a tensor's data_ptr() to the library, which is NULL for an empty tensor and refused there, so the runs through
FusedRAdam take the 47 non-empty tensors of the 48-tensor shape (the update is element by element, the tensor's index changes
nothing); the guarded entry points at all 48 tensors, the empty one included, are called through the C ABI."""
import contextlib
import ctypes as C

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, ops
from tests import optimizer_reference as O
from tests.helpers import _POISON

pytestmark = pytest.mark.gpu
TAIL = 64
MIXED = [90880, 0, 1, 255, 256, 257, 65537, 3, 4099, 64, 1000, 8192]  # then 36 small ones: _mixed_sizes
NO_GRAD = (2, 5, 11, 47)  # tensors of the 48-tensor launch whose gradient is NULL


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


def _mixed_sizes():
    return MIXED + [17 + 29 * k for k in range(48 - len(MIXED))]


def _buffers(states, dev):
    """p, g, m, v of every tensor in a poisoned buffer of n + 64 elements -> {name: [buffer per tensor]}."""
    it, pattern = _POISON[torch.float32]
    out = {}
    for name in ("p", "g", "m", "v"):
        out[name] = []
        for st in states:
            buf = torch.empty(st["n"] + TAIL, device=dev)
            buf.view(it).fill_(pattern)
            buf[: st["n"]] = st[name].to(dev)
            out[name].append(buf)
    return out


def _ptrs(bufs, null=()):
    arr = (C.c_void_p * len(bufs))()
    for i, b in enumerate(bufs):
        arr[i] = None if i in null else b.data_ptr()  # the buffer's own pointer: an empty tensor still has its 64-element tail
    return arr


def _launch(states, bufs, t, lr, eps, null=(), n_tensors=None):
    lib = _abi.load_library()
    sizes = (C.c_int32 * len(states))(*[st["n"] for st in states])
    return lib.rsn_radam_step(len(states) if n_tensors is None else n_tensors, _ptrs(bufs["p"]), _ptrs(bufs["g"], null), _ptrs(bufs["m"]),
                              _ptrs(bufs["v"]), sizes, t, lr, O.BETAS[0], O.BETAS[1], eps, ops._stream())


def _tails_intact(label, states, bufs):
    it, pattern = _POISON[torch.float32]
    for name, lst in bufs.items():
        for k, (st, b) in enumerate(zip(states, lst)):
            assert bool((b[st["n"]:].view(it) == pattern).all()), f"{label}: the tail behind {name} of tensor {k} ({st['n']} elements) was written"


def _judge(label, pool, states, bufs, t, lr, eps, skip=(), coef=None):
    """states: slices of `pool` (optimizer_reference.slice_state), one per tensor of the launch."""
    pieces = [(st["offset"], tuple(bufs[q][k][: st["n"]].cpu() for q in ("p", "m", "v"))) for k, st in enumerate(states) if k not in skip]
    vs = O.judge_pieces(label, pool, t, lr, eps, pieces, coef)
    text = O.report(vs)
    print(f"SHARE {label} {O.worst_share(vs):.3f}\n" + text)
    for v in vs:
        for r in v.rows:
            if not r["ok"]:
                k = max(i for i, st in enumerate(states) if st["offset"] <= r["point"])
                text += f"\n{r['quantity']} {r['cls']}: element {r['point'] - states[k]['offset']} of tensor {k} ({states[k]['n']} elements)"
    assert all(v.ok for v in vs), "\n" + "\n".join(line for line in text.split("\n") if "FAIL" in line or "element" in line)


def _unchanged(label, states, bufs, which):
    for k in which:
        st = states[k]
        for name in ("p", "m", "v", "g"):
            assert torch.equal(bufs[name][k][: st["n"]].cpu().view(torch.int32), st[name].view(torch.int32)), f"{label}: {name} of tensor {k} changed"


@pytest.mark.parametrize("eps", O.EPSS, ids=lambda e: f"eps{e:.0e}")
@pytest.mark.parametrize("lr", O.LRS, ids=lambda x: f"lr{x:.0e}")
@pytest.mark.parametrize("t", O.STEPS)
def test_single_step_against_fp64(dev, t, lr, eps):
    """Two tensors of 4,099 elements in one launch: moments of a previous step, and fresh zero moments."""
    pools = [O.make_state(4099, 11), O.make_state(4099, 12, fresh=True)]
    states = [O.slice_state(p, 0, 4099) for p in pools]
    bufs = _buffers(states, dev)
    with _launching():
        _abi.check(_launch(states, bufs, t, lr, eps))
    label = f"t{t} lr{lr:.0e} eps{eps:.0e}"
    _tails_intact(label, states, bufs)
    for k, st in enumerate(states):
        assert torch.equal(bufs["g"][k][: st["n"]].cpu(), st["g"]), "the gradient is an input"
        _judge(f"{label} {'fresh' if k else 'previous'} moments", pools[k], [st], {q: [b[k]] for q, b in bufs.items()}, t, lr, eps)


def _pool():
    """The state every single-tensor launch takes its first n elements from: a tensor of one element is then held to the bound of
    its class over 90,880 elements, not to the oracle's luck on that element."""
    return O.make_state(max(O.SIZES), 20)


_SIZE_RESULTS = {}  # size -> (p, m, v) bits of the unguarded launch, for the guarded comparison


@pytest.mark.parametrize("n", O.SIZES)
def test_one_tensor_of_each_size(dev, n):
    t, lr, eps = 7, O.LRS[0], O.EPSS[0]
    states = [O.slice_state(_pool(), 0, n)]
    bufs = _buffers(states, dev)
    with _launching():
        _abi.check(_launch(states, bufs, t, lr, eps))
    _tails_intact(f"n{n}", states, bufs)
    _judge(f"n{n} t{t}", _pool(), states, bufs, t, lr, eps)
    _SIZE_RESULTS[n] = tuple(bufs[k][0][:n].cpu() for k in ("p", "m", "v"))


def _mixed_states():
    """The 48 tensors as consecutive slices of one state, so that they are judged together, per gradient decade."""
    sizes = _mixed_sizes()
    pool = O.make_state(sum(sizes), 40)
    offs = [sum(sizes[:k]) for k in range(len(sizes))]
    return pool, [O.slice_state(pool, a, a + n) for a, n in zip(offs, sizes)]


_MIXED_RESULT = {}


def test_48_tensors_in_one_launch(dev):
    """The limit of one launch: mixed sizes with an empty tensor and the 90,880-element one, four tensors without a gradient (their
    p, m and v keep their bits), every tail intact."""
    t, lr, eps = 1000, O.LRS[0], O.EPSS[1]
    pool, states = _mixed_states()
    assert len(states) == 48 and 0 in _mixed_sizes() and max(_mixed_sizes()) == 90880
    bufs = _buffers(states, dev)
    with _launching():
        _abi.check(_launch(states, bufs, t, lr, eps, null=NO_GRAD))
    _tails_intact("48 tensors", states, bufs)
    _unchanged("48 tensors", states, bufs, NO_GRAD)
    _judge("48 tensors t1000", pool, states, bufs, t, lr, eps, skip=NO_GRAD)
    _MIXED_RESULT["bits"] = [tuple(bufs[k][i][: st["n"]].cpu() for k in ("p", "m", "v")) for i, st in enumerate(states)]


def test_refusals_write_nothing(dev):
    """49 tensors and step 0: RSN_ERR_INVALID_ARGUMENT, and no buffer changes."""
    lib = _abi.load_library()
    states = [O.make_state(17 + k, 90 + k) for k in range(49)]
    bufs = _buffers(states, dev)
    with _launching():
        rc49 = _launch(states, bufs, 7, O.LRS[0], O.EPSS[0])
        msg49 = lib.rsn_last_error()
        rc0 = _launch(states[:3], {k: v[:3] for k, v in bufs.items()}, 0, O.LRS[0], O.EPSS[0])
        msg0 = lib.rsn_last_error()
    assert rc49 == -1 and b"n_tensors=49" in msg49, (rc49, msg49)  # RSN_ERR_INVALID_ARGUMENT (include/rsn.h)
    assert rc0 == -1 and b"step" in msg0, (rc0, msg0)
    _tails_intact("refusals", states, bufs)
    _unchanged("refusals", states, bufs, range(49))


def _fused(states, bufs, t, lr, eps, no_grad=(), **guard):
    """FusedRAdam on views of the poisoned buffers, at step t - 1 with the states' moments."""
    params = []
    for k, st in enumerate(states):
        p = torch.nn.Parameter(bufs["p"][k][: st["n"]])
        p.grad = None if k in no_grad else bufs["g"][k][: st["n"]]
        params.append(p)
    opt = pkg.FusedRAdam(params, lr=lr, betas=O.BETAS, eps=eps, **guard)
    opt.exp_avg = [bufs["m"][k][: st["n"]] for k, st in enumerate(states)]
    opt.exp_avg_sq = [bufs["v"][k][: st["n"]] for k, st in enumerate(states)]
    opt.step_count = t - 1
    return opt


def _bit_equal(label, states, bufs, want):
    for k, st in enumerate(states):
        for name, ref in zip(("p", "m", "v"), want[k]):
            got = bufs[name][k][: st["n"]].cpu()
            assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{label}: {name} of tensor {k} ({st['n']} elements) differs in its bits"


@pytest.mark.parametrize("n", O.SIZES)
def test_guard_that_does_not_clip_is_bit_equal_one_tensor(dev, n):
    """FusedRAdam(max_grad_norm=inf, skip_nonfinite=True): two launches, the same bits as rsn_radam_step."""
    t, lr, eps = 7, O.LRS[0], O.EPSS[0]
    states = [O.slice_state(_pool(), 0, n)]
    if n not in _SIZE_RESULTS:  # run alone: the unguarded launch first
        bufs = _buffers(states, dev)
        with _launching():
            _abi.check(_launch(states, bufs, t, lr, eps))
        _SIZE_RESULTS[n] = tuple(bufs[k][0][:n].cpu() for k in ("p", "m", "v"))
    bufs = _buffers(states, dev)
    opt = _fused(states, bufs, t, lr, eps, max_grad_norm=float("inf"), skip_nonfinite=True)
    with _launching():
        opt.step()
    stats = opt.guard_stats()
    assert stats["last_coef"] == 1.0 and not stats["last_skipped"] and opt.step_count == t
    _tails_intact(f"guarded n{n}", states, bufs)
    _bit_equal(f"guarded n{n}", states, bufs, [_SIZE_RESULTS[n]])


def _non_empty(states):
    keep = [k for k, st in enumerate(states) if st["n"] > 0]
    return keep, [states[k] for k in keep]


def test_guard_that_does_not_clip_is_bit_equal_mixed_tensors(dev):
    t, lr, eps = 1000, O.LRS[0], O.EPSS[1]
    pool, all_states = _mixed_states()
    if "bits" not in _MIXED_RESULT:
        bufs = _buffers(all_states, dev)
        with _launching():
            _abi.check(_launch(all_states, bufs, t, lr, eps, null=NO_GRAD))
        _MIXED_RESULT["bits"] = [tuple(bufs[k][i][: st["n"]].cpu() for k in ("p", "m", "v")) for i, st in enumerate(all_states)]
    keep, states = _non_empty(all_states)
    no_grad = tuple(i for i, k in enumerate(keep) if k in NO_GRAD)
    assert len(states) == 47 and len(no_grad) == len(NO_GRAD)
    bufs = _buffers(states, dev)
    opt = _fused(states, bufs, t, lr, eps, no_grad=no_grad, max_grad_norm=float("inf"), skip_nonfinite=True)
    with _launching():
        opt.step()
    assert opt.guard_stats()["last_coef"] == 1.0
    _tails_intact("guarded 47 tensors", states, bufs)
    _unchanged("guarded 47 tensors", states, bufs, no_grad)
    _bit_equal("guarded 47 tensors", states, bufs, [_MIXED_RESULT["bits"][k] for k in keep])


def test_guarded_entry_points_at_48_tensors_are_bit_equal(dev):
    """rsn_grad_sumsq + rsn_radam_step_guarded through the C ABI at the limit of 48 tensors, the empty one and the four without a
    gradient included (FusedRAdam cannot pass an empty tensor): no clipping, skip_nonfinite on -> the bits of rsn_radam_step."""
    lib = _abi.load_library()
    t, lr, eps = 1000, O.LRS[0], O.EPSS[1]
    pool, states = _mixed_states()
    if "bits" not in _MIXED_RESULT:
        bufs = _buffers(states, dev)
        with _launching():
            _abi.check(_launch(states, bufs, t, lr, eps, null=NO_GRAD))
        _MIXED_RESULT["bits"] = [tuple(bufs[k][i][: st["n"]].cpu() for k in ("p", "m", "v")) for i, st in enumerate(states)]
    bufs = _buffers(states, dev)
    n = len(states)
    sizes = (C.c_int32 * n)(*[st["n"] for st in states])
    nbytes = lib.rsn_grad_sumsq_workspace_bytes(n, sizes)
    assert n == 48 and nbytes >= 48 * 8
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    stats = torch.zeros(C.sizeof(_abi.GuardStats) // 4, dtype=torch.int32, device=dev)
    grads = _ptrs(bufs["g"], NO_GRAD)
    with _launching():
        _abi.check(lib.rsn_grad_sumsq(n, grads, sizes, C.c_void_p(ws.data_ptr()), nbytes, ops._stream()))
        _abi.check(lib.rsn_radam_step_guarded(n, _ptrs(bufs["p"]), grads, _ptrs(bufs["m"]), _ptrs(bufs["v"]), sizes, t, lr, O.BETAS[0], O.BETAS[1],
                                              eps, 0.0, 1, C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(stats.data_ptr()), ops._stream()))
    st = _abi.GuardStats.from_buffer_copy(stats.cpu().numpy().tobytes())
    assert float(st.last_coef) == 1.0 and int(st.last_skipped) == 0
    _tails_intact("guarded 48 tensors", states, bufs)
    _unchanged("guarded 48 tensors", states, bufs, NO_GRAD)
    _bit_equal("guarded 48 tensors", states, bufs, _MIXED_RESULT["bits"])


def test_clipped_step_against_fp64(dev):
    """One clipped step at the mixed-tensor shape: the update reads g * coef, coef as the kernel recorded it (guard_stats), which is
    itself checked against max_norm / (norm + 1e-6) of the fp64 norm; p, m and v by the rule with g * coef in the reference."""
    t, lr, eps, max_norm = 1000, O.LRS[0], O.EPSS[1], 100.0  # coef about 1e-3: (1 - beta2) (g coef)^2 stays a normal number
    pool, all_states = _mixed_states()
    keep, states = _non_empty(all_states)
    no_grad = tuple(i for i, k in enumerate(keep) if k in NO_GRAD)
    bufs = _buffers(states, dev)
    opt = _fused(states, bufs, t, lr, eps, no_grad=no_grad, max_grad_norm=max_norm)
    with _launching():
        opt.step()
    stats = opt.guard_stats()
    norm = sum(float((st["g"].double() ** 2).sum()) for i, st in enumerate(states) if i not in no_grad) ** 0.5
    coef = stats["last_coef"]
    print(f"clipped step: norm {norm:.6e} (kernel {stats['last_norm']:.6e}), coef {coef:.6e}")
    assert 0.0 < coef < 1.0 and abs(stats["last_norm"] - norm) <= 2.0 ** -22 * norm
    assert abs(coef - max_norm / (norm + 1e-6)) <= 2.0 ** -21 * coef  # the norm's rounding, the sum and the division in float32
    _tails_intact("clipped", states, bufs)
    _unchanged("clipped", states, bufs, no_grad)
    _judge("clipped 47 tensors t1000", pool, states, bufs, t, lr, eps, skip=no_grad, coef=coef)
