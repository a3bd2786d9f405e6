"""Weight gradients (rsn_wgrad.hip) bit for bit: every kernel variant, both flushes and every entry point on the integer operand
classes of tests/wgrad_cases.py, where the fp64 result is exact in any order of addition -- the atomics' included -- and in each of
the kernel's arithmetics.  tests/test_wgrad_exact_cpu.py proves on the host that each class tells a correct reduction from one that
has lost or misplaced one of its six piece products, a point, a row or a column; here every integer assertion is a torch.equal
against the fp64 reference cast to float32, over the WHOLE destination buffer (what a call must leave alone is part of it).

  1. variants: NKB 2, 4, 8 x row-block splits P 1, 2, 4 x the three load layouts (vector / vector, vector X beside <= 32 outputs or
     scalar dY, scalar / scalar: by shape, and by an X pointer 4 bytes off an aligned shape), f32 and bf16x6 on A, B, C and D, bf16 on
     D, atomic and ordered flush (the ordered one over a NaN-filled workspace).  Five segments: one empty, one below a stage, ragged
     boundaries (vprefix shifts the round-robin deal).  dW lies at a column offset in a wider and taller buffer that holds integers
     already: the call accumulates, and the columns in front, the columns behind and the rows from n_out on keep their values.
  2. the two statements of the six-product stage, separately: segments that are multiples of 16 points (x6_stage alone), searched on
     the host so that the wave slots' stage counts cover 0, 1, 2, 3 and at least 4 (the pair loop, the odd leftover, an even count)
     for the grid the launcher really takes -- read off the refusal of an ordered call without workspace -- and one segment of 15
     points (mma_stage alone).
  3. eight segments, device-side counts below the bound, 0 and above it (clamped) with more than one row per count.
  4. a column map that permutes and drops columns.
  5. rsn_weight_grad_jobs / _ordered with 2 and 5 jobs on different operands per job.
  6. rows that are bf16 in memory (class D).
  7. random fp32 operands judged entry by entry: |got - fp64| <= K 2^-24 S[n, k], S = |dy|^T |x|, K = 4 x the worst ratio of a
     float32 restatement on the host (wgrad_cases.random_case).  This is per-entry coverage of real roundings (small entries, edge
     rows); it is NOT what detects a dropped product -- a dropped small product moves an entry by about 3 x 2^-24 S, inside any such
     margin -- items 1 and 2 are.
No constant here comes from a run of the kernels."""
import collections
import ctypes as C
import re

import pytest
import torch

import reflect_sampling_nerf_amd as pkg
from reflect_sampling_nerf_amd import _abi, train_graph
from tests import test_deterministic_gpu as DT
from tests import wgrad_cases as W

pytestmark = pytest.mark.gpu

MODES = DT.MODES
FLUSHES = ("atomic", "ordered")
BF = torch.bfloat16
COL0, BEHIND, ROWS_BEHIND = 5, 3, 2  # dW's place in its buffer: columns in front / behind, rows behind


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg.load_library()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------- helpers
def _rows(dev, t, offset=0, dtype=None):
    """t [n, ld] on the device as a view that starts `offset` elements into its allocation (the rows stay inside it)."""
    flat = torch.full((t.numel() + offset,), W.PAD, dtype=dtype or t.dtype, device=dev)
    flat[offset:] = t.to(dev).to(flat.dtype).reshape(-1)
    return flat[offset:].view(t.shape[0], t.shape[1])


def _segments(dev, c, lens, x_off=0, dy_dtype=None, x_dtype=None, counts=None):
    """The case's points as consecutive segments of the given lengths; counts: {segment: (device count tensor, rows per count)}."""
    segs, m0 = [], 0
    for s, n in enumerate(lens):
        sg = (_rows(dev, c.dy[m0:m0 + n], 0, dy_dtype), _rows(dev, c.x[m0:m0 + n], x_off, x_dtype))
        segs.append(sg + (counts[s],) if counts and s in counts else sg)
        m0 += n
    assert m0 == c.dy.shape[0]
    return segs


def _prior(rows, cols, salt=0):
    """The integers a destination holds before the call."""
    i, j = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    return ((i * 7 + j * 3 + salt * 11) % 41 - 20).float()


class _Dest:
    """dW [n_out, k_in] at column COL0 of a wider, taller buffer of integers, db likewise in a longer vector."""

    def __init__(self, dev, n_out, k_in, want_db, width=None, salt=0):
        self.n_out, self.k_in = n_out, k_in
        self.w0 = _prior(n_out + ROWS_BEHIND, COL0 + (width or k_in) + BEHIND, salt)
        self.b0 = _prior(1, n_out + ROWS_BEHIND, salt + 1)[0]
        self.dw, self.db = self.w0.clone().to(dev), (self.b0.clone().to(dev) if want_db else None)

    def check(self, label, ref_w, ref_b, col_map=None):
        exp = self.w0.double()
        if col_map is None:
            exp[:self.n_out, COL0:COL0 + self.k_in] += ref_w
        else:
            for k, c in enumerate(col_map):
                if c >= 0:
                    exp[:self.n_out, COL0 + c] += ref_w[:, k]
        assert float(exp.abs().max()) < W.EXACT
        got = self.dw.cpu()
        if not torch.equal(got, exp.float()):
            bad = (got != exp.float())
            inside = bad[:self.n_out, COL0:COL0 + (exp.shape[1] - COL0 - BEHIND)]
            raise AssertionError(f"{label}: dW differs from the fp64 sums in {int(bad.sum())} elements ({int(bad.sum()) - int(inside.sum())} of them "
                                 f"outside the destination), worst by {float((got.double() - exp).abs().max()):.0f}")
        if self.db is not None:
            eb = self.b0.double()
            eb[:self.n_out] += ref_b
            assert torch.equal(self.db.cpu(), eb.float()), f"{label}: db differs from the fp64 sums"


def _launch(flush, segs, n_out, k_in, dw, col0, db, mode, col_map=None):
    if flush == "atomic":
        train_graph._wgrad_multi(segs, n_out, k_in, dw, col0, db, col_map, mode=MODES[mode], ordered=False)
    else:
        need = DT._ws_bytes(segs, 1, n_out, k_in, MODES[mode])
        rc = DT.ordered_multi(segs, n_out, k_in, dw, col0, db, MODES[mode], DT._workspace(dw.device, need, float("nan")), col_map=col_map)
        assert rc == 0, pkg.load_library().rsn_last_error()


def _modes(cls):
    return ("f32", "bf16x6", "bf16") if cls == "D" else ("f32", "bf16x6")


def _run_case(dev, label, c, segs, flush, modes, rows=None, col_map=None, width=None):
    """One call per mode into a fresh destination; db where the host can assert its sums exact (class A: db = NULL, a path of its own)."""
    want_db = c.db_exact(rows)
    c.assert_meaningful(rows, want_db=want_db, label=label)
    ref_w, ref_b = c.reference(rows)
    cm = None if col_map is None else torch.tensor(col_map, dtype=torch.int32, device=dev)
    for mode in modes:
        d = _Dest(dev, c.n_out, c.k_in, want_db, width)
        _launch(flush, segs, c.n_out, c.k_in, d.dw, COL0, d.db, mode, cm)
        d.check(f"{label} {mode} {flush}", ref_w, ref_b, col_map)


# ---------------------------------------------------------------------------------------------- 1. variants
@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("cls", W.CLASSES)
@pytest.mark.parametrize("n_out,k_in,ld_dy,ld_x,x_off", W.VARIANT_SHAPES, ids=[W.shape_id(s) for s in W.VARIANT_SHAPES])
def test_every_variant_returns_the_integer_sums(dev, n_out, k_in, ld_dy, ld_x, x_off, cls, flush):
    c = W.case(cls, sum(W.SEG_LENS), n_out, k_in, ld_dy, ld_x)
    segs = _segments(dev, c, W.SEG_LENS, x_off)
    assert x_off == 0 or all(sg[1].data_ptr() % 16 == 4 * x_off for sg in segs if sg[1].shape[0])
    _run_case(dev, W.shape_id((n_out, k_in, ld_dy, ld_x, x_off)), c, segs, flush, _modes(cls))


# ---------------------------------------------------------------------------------------------- 2. the two six-product stages
def launch_grid(dev, lens, n_out, k_in, ld_dy, ld_x, mode):
    """Workgroups of the launch for segments of these lengths (rows and pointers on the vector-load layout), as
    tools/record_wgrad_errors.py reads them: an ordered call with workspace_bytes = 0 is refused before any launch and
    rsn_last_error() names the bytes.  Nothing is dereferenced, so one small allocation stands for every pointer."""
    lib = pkg.load_library()
    ns = len(lens)
    buf = torch.empty(64, device=dev)
    assert buf.data_ptr() % 16 == 0
    ptrs = (C.c_void_p * ns)(*[buf.data_ptr()] * ns)
    rc = lib.rsn_weight_grad_multi_dev_ordered(ns, (C.c_int64 * ns)(*lens), (C.c_void_p * ns)(), (C.c_int32 * ns)(*[1] * ns), ptrs, ld_dy, n_out,
                                               ptrs, ld_x, k_in, None, _abi.ptr(buf), k_in, None, MODES[mode], 0, _abi.ptr(buf), 0, None)
    m = re.search(r"needs (\d+) bytes", lib.rsn_last_error().decode())
    assert rc == -1 and m, (rc, lib.rsn_last_error())
    return W.grid_of_workspace_bytes(int(m.group(1)), k_in)


def _histogram(lens, G, step):
    deal = W.slot_stages(lens, G, step)
    h = collections.Counter(c for row in deal for c, _ in row)
    return dict(sorted(h.items())), sum(t for row in deal for _, t in row)


@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("cls", ("A", "B", "C"))
@pytest.mark.parametrize("n_out,k_in", W.STAGE_SHAPES)
def test_full_stages_only_run_the_main_loop(dev, n_out, k_in, cls, flush):
    """Segments of whole 16-point stages: no masked tail stage anywhere, so x6_stage (splits carried across stages) multiplies
    every point of the split-bf16 run.  The lengths come from a host search (wgrad_cases.full_stage_lengths) against the grid the
    launcher takes on THIS device; the deal restated for that grid must give some (slot, segment) 0, 1, 2, 3 and >= 4 stages."""
    nsub = W.nsub_of(n_out)
    lens, G = W.full_stage_lengths(lambda ls: launch_grid(dev, ls, n_out, k_in, n_out, k_in, "bf16x6"), nsub)
    assert all(n % 16 == 0 for n in lens)
    seen, tails = W.counts_seen(lens, G, 16)
    print(f"{n_out}x{k_in} bf16x6: segments {lens}, {G} wave slots, (slot, segment) stage counts {_histogram(lens, G, 16)[0]}, {tails} tail stages")
    assert seen == {0, 1, 2, 3, 4} and tails == 0
    G32 = launch_grid(dev, lens, n_out, k_in, n_out, k_in, "f32") * nsub
    print(f"{n_out}x{k_in} f32 (8-point stages): {G32} wave slots, stage counts {_histogram(lens, G32, 8)[0]}")
    c = W.case(cls, sum(lens), n_out, k_in)
    _run_case(dev, f"full stages {n_out}x{k_in}", c, _segments(dev, c, lens), flush, ("bf16x6", "f32"))


@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("cls", ("A", "B", "C"))
@pytest.mark.parametrize("n_out,k_in", W.STAGE_SHAPES)
def test_one_tail_stage_alone(dev, n_out, k_in, cls, flush):
    """One segment of 15 points: below a 16-point stage, so the split-bf16 run is mma_stage's masked tail alone (one wave slot per
    row-block pair; every other slot idle).  The fp32 kernel takes one full 8-point stage and a tail of 7."""
    c = W.case(cls, W.TAIL_POINTS, n_out, k_in)
    assert W.counts_seen([W.TAIL_POINTS], 4, 16) == ({0}, 1)
    _run_case(dev, f"tail only {n_out}x{k_in}", c, _segments(dev, c, [W.TAIL_POINTS]), flush, ("bf16x6", "f32"))


# ---------------------------------------------------------------------------------------------- 3. segments and counts
@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("n_out,k_in,ld_dy,ld_x", W.COUNT_SHAPES)
def test_eight_segments_and_device_counts(dev, n_out, k_in, ld_dy, ld_x, flush):
    """Eight segments (WG_MAX_SEG), three cut by a device-side count with several rows per count: below the bound, 0, and above the
    bound (the kernel clamps to the segment's rows).  Class D: any subset of its points is a case."""
    c = W.case("D", sum(W.EIGHT_LENS), n_out, k_in, ld_dy, ld_x)
    counts = {s: (torch.tensor([cnt], dtype=torch.int32, device=dev), per) for s, (cnt, per) in W.EIGHT_COUNTS.items()}
    rows = W.live_rows(W.EIGHT_LENS, W.EIGHT_COUNTS)
    assert 0 < rows.numel() < sum(W.EIGHT_LENS)
    _run_case(dev, f"eight segments {n_out}x{k_in}", c, _segments(dev, c, W.EIGHT_LENS, counts=counts), flush, _modes("D"), rows=rows)


# ---------------------------------------------------------------------------------------------- 4. column map
@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("cls", ("B", "D"))
def test_column_map_permutes_and_drops(dev, cls, flush):
    """256 x 104 through a col_map into a 120-column window: a permutation with every 13th packed column dropped (-1).  The columns
    of the window that the map does not reach keep their integers."""
    n_out, k_in = 256, 104
    cmap = W.column_map(k_in, W.MAP_WIDTH)
    c = W.case(cls, sum(W.SEG_LENS), n_out, k_in)
    _run_case(dev, f"col_map {n_out}x{k_in}", c, _segments(dev, c, W.SEG_LENS), flush, _modes(cls), col_map=cmap, width=W.MAP_WIDTH)


# ---------------------------------------------------------------------------------------------- 5. jobs
@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("cls", ("A", "B"))
@pytest.mark.parametrize("n_jobs,n_out,k_in", [(2, 256, 256), (5, 256, 256), (2, 128, 104), (5, 64, 64)])
def test_jobs_each_return_their_own_sums(dev, n_jobs, n_out, k_in, cls, flush):
    """rsn_weight_grad_jobs / rsn_weight_grad_jobs_ordered: every job has operands of its own (another salt) and must return its
    own reference, so a workgroup that reads another job's rows or flushes into another job's dW shows.  The middle segment is empty
    (the ordered call hands it to the library as it is; the atomic wrapper drops it)."""
    cases = [W.case(cls, sum(W.JOB_LENS), n_out, k_in, salt=7 + jb) for jb in range(n_jobs)]
    refs = []
    for jb, c in enumerate(cases):
        c.assert_meaningful(want_db=c.db_exact(), label=f"job {jb}")
        refs.append(c.reference())
        assert jb == 0 or not torch.equal(refs[jb][0], refs[0][0])
    for mode in _modes(cls):
        dests = [_Dest(dev, n_out, k_in, c.db_exact(), salt=jb) for jb, c in enumerate(cases)]
        jobs = [(_segments(dev, c, W.JOB_LENS), d.dw, COL0, d.db, None) for c, d in zip(cases, dests)]
        if flush == "atomic":
            train_graph._wgrad_jobs(jobs, n_out, k_in, mode=MODES[mode], ordered=False)
        else:
            need = DT._ws_bytes(jobs[0][0], n_jobs, n_out, k_in, MODES[mode])
            assert DT.ordered_jobs(jobs, n_out, k_in, MODES[mode], DT._workspace(dev, need, float("nan"))) == 0, pkg.load_library().rsn_last_error()
        for jb, (d, (ref_w, ref_b)) in enumerate(zip(dests, refs)):
            d.check(f"job {jb} of {n_jobs} {n_out}x{k_in} {mode} {flush}", ref_w, ref_b)


# ---------------------------------------------------------------------------------------------- 6. bf16 rows in memory
@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("n_out,k_in,ld_dy,x_bf16,dy_bf16", W.BF16_ROW_SHAPES)
def test_bf16_rows_in_memory(dev, n_out, k_in, ld_dy, x_bf16, dy_bf16, flush):
    """Class D as rows that ARE bf16 in memory (|v| <= 15: the same values), plain bf16 mode: X and dY rows, dY rows beside fp32 X,
    X rows beside fp32 dY of at most 32 outputs -- for each NKB."""
    c = W.case("D", sum(W.SEG_LENS), n_out, k_in, ld_dy, k_in)
    segs = _segments(dev, c, W.SEG_LENS, dy_dtype=BF if dy_bf16 else None, x_dtype=BF if x_bf16 else None)
    _run_case(dev, f"bf16 rows {n_out}x{k_in} x={x_bf16} dy={dy_bf16}", c, segs, flush, ("bf16",))


# ---------------------------------------------------------------------------------------------- 7. random operands, entry by entry
def random_ratio(dev, mode, n_out, k_in, ld_dy, ld_x, flush):
    """-> (worst |got - fp64| / (2^-24 S) over the entries, K of the host restatement) of one random case."""
    vector = n_out > 32 and k_in % W.nkb_of(k_in) == 0 and ld_x % min(4, W.nkb_of(k_in)) == 0 and ld_dy % 2 == 0
    r = W.random_case(sum(DT.LENS), n_out, k_in, ld_dy, ld_x, rounded=(mode == "bf16" and vector))
    segs, m0 = [], 0
    for n in DT.LENS:
        segs.append((r["dy"][m0:m0 + n].to(dev), r["x"][m0:m0 + n].to(dev)))
        m0 += n
    dw = torch.zeros(n_out, k_in, device=dev)
    _launch(flush, segs, n_out, k_in, dw, 0, None, mode)
    assert bool(torch.isfinite(dw).all())
    return float(((dw.double().cpu() - r["ref"]).abs() / (W.ULP * r["S"])).max()), r["K"]


@pytest.mark.parametrize("flush", FLUSHES)
@pytest.mark.parametrize("mode,n_out,k_in,ld_dy,ld_x", W.RANDOM_CASES)
def test_random_operands_entry_by_entry(dev, mode, n_out, k_in, ld_dy, ld_x, flush):
    """randn operands, 6043 points in five segments: every entry within K 2^-24 S[n, k] of fp64 (plain bf16 on its vector path: of
    the bf16-rounded operands' product).  Per-entry coverage -- a small entry beside large ones, edge rows -- of real fp32
    roundings; a dropped piece product stays inside this margin and is caught by the integer cases above, not here."""
    ratio, K = random_ratio(dev, mode, n_out, k_in, ld_dy, ld_x, flush)
    print(f"random {mode} {n_out}x{k_in} {flush}: worst |err| = {ratio:.3f} x 2^-24 S, bound K = {K:.3f} (4 x the float32 restatement's)")
    assert ratio <= K
