"""The operand classes, references and host-side checks of tests/test_wgrad_exact_gpu.py (weight gradients of rsn_wgrad.hip, bit for
bit), stated once for that file, for tests/test_wgrad_exact_cpu.py -- which proves every case meaningful before a GPU sees it -- and
for tools/wgrad_exact_report.py.  Host only: no library call, no GPU.

dW[n][k] = sum_m dY[m][n] X[m][k] and db[n] = sum_m dY[m][n] over small INTEGERS: every product and every partial sum is an integer
below 2^24, so the sum is exact in any order and in any of the kernel's arithmetics (fp32 MFMA, six bf16 piece products, one bf16
product, fp32 atomics, the ordered reducer), and a kernel that is right returns the fp64 result bit for bit.  The split-bf16 kernel
forms the pieces h = bf16(v), m = bf16(v - h), l = bf16(v - h - m) (nearest even: split2) and keeps six products (mma6, KEPT below).

  A  wide dY x unit X   |dy| in [2^18, 2^19): hi, mid and lo non-zero; x in {0, +1, -1}.    Carried by hi hi, mid hi, lo hi.
  B  unit dY x wide X   the mirror.                                                        Carried by hi hi, hi mid, hi lo.
  C  two-piece x two-piece   both in [2^9, 2^10): hi and mid non-zero, lo zero.            Carried by mid mid, hi mid, mid hi, hi hi.
  D  one-piece x one-piece   |v| <= 15, dense: exact in plain bf16 and as rows that are bf16 in memory; the class for launch
     geometry, where many points are needed.

A, B and C are sparse so that the sums stay in range: the points are dealt round-robin to qr x qk (row residue, column residue)
pairs, point m being non-zero in the rows n with n % qr == rr(m) and the columns k with k % qk == rk(m) only.  Every output element
then receives ceil or floor of points / (qr qk) contributions, at least 1 and at most CONTRIBUTIONS[class]:
30 x 2^19 x 1.01^2 < 2^24 (A, B) and 15 x 2^20 x 1.01^2 < 2^24 (C) -- 1.01^2 is the project's rule (tests/depth_skip_cases.py): the
pieces of an integer are integers whose magnitudes sum to less than 1.01 times the value's.

No constant here comes from a run of the kernels."""
import functools
import math

import torch

f32, f64 = torch.float32, torch.float64
EXACT = 2.0 ** 24
PIECES = 1.01 ** 2
CLASSES = ("A", "B", "C", "D")
CONTRIBUTIONS = {"A": 30, "B": 30, "C": 15}
PAD = 5.0  # what the columns between n_out / k_in and the leading dimension hold: read by no live lane, flushed by none
# mma6's products (piece of dY, piece of X; 0 = hi, 1 = mid, 2 = lo), in its order: a3 b1, a2 b2, a1 b3, a2 b1, a1 b2, a1 b1
KEPT = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
PIECE = ("hi", "mid", "lo")
# the product each class is built for, and what carries its sum
BUILT_FOR = {"A": (2, 0), "B": (0, 2), "C": (1, 1)}
CARRIED_BY = {"A": ((0, 0), (1, 0), (2, 0)), "B": ((0, 0), (0, 1), (0, 2)), "C": ((0, 0), (0, 1), (1, 0), (1, 1)), "D": ((0, 0),)}


def name(product):
    return f"{PIECE[product[0]]} x {PIECE[product[1]]}"


def pieces(v):
    """(hi, mid, lo) of float32 v as split2 forms them: bf16 roundings to nearest even of v, v - hi, v - hi - mid (the
    subtractions are exact in float32)."""
    v = v.to(f32)
    h = v.bfloat16().to(f32)
    m = (v - h).bfloat16().to(f32)
    return h, m, (v - h - m).bfloat16().to(f32)


def six_products(a, b, products=KEPT):
    """The split-bf16 reduction restated in fp64: sum over `products` of (piece of a)^T (piece of b); a [M, N], b [M, K]."""
    pa, pb = [p.double() for p in pieces(a)], [p.double() for p in pieces(b)]
    out = torch.zeros(a.shape[1], b.shape[1], dtype=f64)
    for i, j in products:
        out += pa[i].t() @ pb[j]
    return out


def without(product):
    return tuple(p for p in KEPT if p != product)


def swapped(product, other):
    return tuple(other if p == product else p for p in KEPT)


def _mix(m, j, salt):
    """A deterministic 24-bit scramble of (point, column, salt): index arithmetic, no generator."""
    h = ((m * 73856093) ^ (j * 19349663) ^ (salt * 83492791 + 12345)) % (1 << 32)  # every product below 2^63
    h = (h * 1664525 + 1013904223) % (1 << 32)
    h = ((h ^ (h >> 15)) * 1103515245) % (1 << 32)
    return (h ^ (h >> 13)) >> 8


def _wide(m, j, salt, lo_bit):
    """Signed integers with magnitude in [2^lo_bit, 2^(lo_bit + 1))."""
    h = _mix(m, j, salt)
    return ((1 << lo_bit) + h % (1 << lo_bit)) * (1 - 2 * ((h >> 20) & 1))


def _unit(m, j, salt):
    return 1 - 2 * (_mix(m, j, salt) & 1)


def moduli(cls, n_pts, n_out, k_in):
    """(qr, qk) of a sparse class: at least one and at most CONTRIBUTIONS[cls] points per output element.  Eight row residues
    (fewer for fewer rows or points), more where the columns alone cannot thin the points out enough."""
    pairs = math.ceil(n_pts / CONTRIBUTIONS[cls])  # (row residue, column residue) pairs needed; 1: a handful of points, dense
    qr = max(1, min(8, n_out, pairs))
    while True:
        qk = math.ceil(pairs / qr)
        if qk <= k_in or qr >= n_out:
            break
        qr = min(2 * qr, n_out)
    assert qk <= k_in and qr * qk <= n_pts, f"class {cls}: {n_pts} points do not fit {n_out} x {k_in} outputs"
    return qr, qk


class Case:
    """Operands dy [M, ld_dy], x [M, ld_x] (float32, integers) of one class; the reduction reads dy[:, :n_out] and x[:, :k_in]."""

    def __init__(self, cls, dy, x, n_out, k_in):
        self.cls, self.dy, self.x, self.n_out, self.k_in = cls, dy, x, n_out, k_in

    def operands(self, rows=None):
        a, b = self.dy[:, :self.n_out], self.x[:, :self.k_in]
        return (a, b) if rows is None else (a[rows], b[rows])

    def reference(self, rows=None):
        """fp64 (dW [n_out, k_in], db [n_out]) over `rows` (an index tensor or a slice; None: every point)."""
        a, b = self.operands(rows)
        return a.double().t() @ b.double(), a.double().sum(0)

    def db_exact(self, rows=None):
        a, _ = self.operands(rows)
        return float(a.abs().double().sum(0).max()) < EXACT

    def assert_meaningful(self, rows=None, want_db=False, label=""):
        """What the host must know before the case goes to a GPU (ISSUE / DESIGN 4.24): the sums are exact in any order and in
        six products, every point and every output element takes part, and a permuted flush would show."""
        a, b = self.operands(rows)
        tag = f"{label} class {self.cls} {self.n_out} x {self.k_in}, {a.shape[0]} points"
        assert a.shape[0] > 0, tag
        assert bool((a == a.round()).all()) and bool((b == b.round()).all()), f"{tag}: not integers"
        s = a.abs().double().t() @ b.abs().double()
        assert float(s.max()) * PIECES < EXACT, f"{tag}: a partial sum may leave the exact range ({float(s.max()):.0f})"
        if want_db:
            assert self.db_exact(rows), f"{tag}: the bias sums may leave the exact range"
        pa, pb = [p.abs().double() for p in pieces(a)], [p.abs().double() for p in pieces(b)]
        for i, j in ((1, 2), (2, 1), (2, 2)):  # the dropped products: a zero factor in every term
            assert float((pa[i].t() @ pb[j]).max()) == 0.0, f"{tag}: the dropped product {name((i, j))} is not zero"
        hits = (a != 0).double().t() @ (b != 0).double()
        assert float(hits.min()) >= 1, f"{tag}: an output element receives no contribution"
        assert bool(((a != 0).any(1) & (b != 0).any(1)).all()), f"{tag}: a point is zero in every live row or column"
        ref, _ = self.reference(rows)
        assert torch.unique(ref, dim=0).shape[0] == ref.shape[0], f"{tag}: two rows of the reference are equal"
        assert torch.unique(ref, dim=1).shape[1] == ref.shape[1], f"{tag}: two columns of the reference are equal"
        want = {"A": ((1, 1, 1), (1, 0, 0)), "B": ((1, 0, 0), (1, 1, 1)), "C": ((1, 1, 0), (1, 1, 0)), "D": ((1, 0, 0), (1, 0, 0))}[self.cls]
        for what, ps, w in (("dY", pa, want[0]), ("X", pb, want[1])):
            for k in range(3):
                assert (float(ps[k].max()) > 0) == bool(w[k]), f"{tag}: the {PIECE[k]} piece of {what} is {'zero' if w[k] else 'not zero'}"
        if self.cls == "D":
            assert bool((a == a.bfloat16().float()).all()) and bool((b == b.bfloat16().float()).all())


@functools.lru_cache(maxsize=None)
def case(cls, n_pts, n_out, k_in, ld_dy=None, ld_x=None, salt=0):
    """The operands of class `cls` for n_pts points (the segments of a call are consecutive row ranges of them).  Cached: shared
    among the tests of a shape, and left unchanged by them."""
    ld_dy, ld_x = ld_dy or n_out, ld_x or k_in
    m = torch.arange(n_pts, dtype=torch.int64)[:, None]
    n, k = torch.arange(ld_dy, dtype=torch.int64)[None, :], torch.arange(ld_x, dtype=torch.int64)[None, :]
    if cls == "D":
        dy, x = _mix(m, n, 2 * salt + 1) % 31 - 15, _mix(m, k, 2 * salt + 2) % 31 - 15
    else:
        qr, qk = moduli(cls, n_pts, n_out, k_in)
        pair = m % (qr * qk)
        live_r, live_k = (n % qr) == (pair % qr), (k % qk) == (pair // qr)
        if cls == "A":
            dy, x = _wide(m, n, 2 * salt + 1, 18), _unit(m, k, 2 * salt + 2)
        elif cls == "B":
            dy, x = _unit(m, n, 2 * salt + 1), _wide(m, k, 2 * salt + 2, 18)
        else:
            dy, x = _wide(m, n, 2 * salt + 1, 9), _wide(m, k, 2 * salt + 2, 9)
        dy, x = dy * live_r, x * live_k
    dy, x = dy.to(f32), x.to(f32)
    dy[:, n_out:], x[:, k_in:] = PAD, PAD
    return Case(cls, dy, x, n_out, k_in)


# ---------------------------------------------------------------------------------------------- the deal of stages to wave slots
def nkb_of(k_in):
    return 8 if k_in > 128 else (4 if k_in > 64 else 2)  # wgrad_nkb


def nsub_of(n_out):
    return 4 // (1 if n_out <= 64 else (2 if n_out <= 128 else 4))  # 4 / wgrad_pairs


def grid_of_workspace_bytes(nbytes, k_in):
    """Workgroups of a launch from the bytes its ordered flush asks for: 4 slots of WG_SLOT_HEAD + 2 NKB 1024 floats a workgroup."""
    per = 16 * (192 + 2048 * nkb_of(k_in))
    assert nbytes % per == 0, (nbytes, per)
    return nbytes // per


def slot_stages(lens, G, step):
    """rsn_wgrad_kernel's deal (`first`, `cnt`, `vprefix`), restated: per wave slot g of G and segment s, (full stages the slot
    multiplies, whether it takes the segment's masked tail stage).  -> [G][segments] of (cnt, tail)."""
    out = [[] for _ in range(G)]
    vprefix = 0
    for n_s in lens:
        n_full, rem = n_s // step, n_s % step
        for g in range(G):
            first = (g - vprefix) % G
            cnt = (n_full - first + G - 1) // G if first < n_full else 0
            out[g].append((cnt, rem > 0 and (vprefix + n_full) % G == g))
        vprefix += n_full + (1 if rem else 0)
    return out


def counts_seen(lens, G, step):
    """The set of per-(slot, segment) full-stage counts, with everything from 4 on folded into 4, and the number of tail stages."""
    deal = slot_stages(lens, G, step)
    return {min(c, 4) for row in deal for c, _ in row}, sum(t for row in deal for _, t in row)


def full_stage_lengths(grid_of, nsub, step=16, tries=32):
    """Three segment lengths, multiples of `step` (no tail stage anywhere), on which the slots' stage counts cover 0, 1, 2, 3 and
    at least 4: with G wave slots and h = max(1, G / 2), segments of 3 G + h, G + h and h stages give the first h slots (after the
    shift by vprefix) 4, 2 and 1 stages and the others 3, 1 and 0.  G follows from the lengths themselves (the grid is the
    launcher's function of the stages and the CU count: grid_of(lens) asks it), so the lengths are searched: start from a guess,
    ask, rebuild, until the deal restated for the grid the launcher really takes covers the set.  -> (lens, G)."""
    G = 4 * nsub
    for _ in range(tries):
        h = max(1, G // 2)
        lens = [step * (3 * G + h), step * (G + h), step * h]
        G_real = grid_of(lens) * nsub
        seen, tails = counts_seen(lens, G_real, step)
        if seen == {0, 1, 2, 3, 4} and tails == 0:
            return lens, G_real
        G = G_real if G_real != G else G + 1
    raise AssertionError("no segment lengths found whose stage counts cover 0, 1, 2, 3 and >= 4")


# ---------------------------------------------------------------------------------------------- random operands, entry by entry
ULP = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def random_case(n_pts, n_out, k_in, ld_dy=None, ld_x=None, rounded=False, seed=0):
    """randn operands and what an entry-wise judgement needs: -> dict(dy, x, ref fp64 dW, S = |dy|^T |x| fp64, ratio32, K).  rounded: the reference and S of the bf16-rounded operands (plain bf16).  ratio32 is the worst
    |restatement - ref| / (2^-24 S) of a float32 restatement on the host -- stage sums of 16 points, added in float32 in the order
    of the points -- and K = 4 ratio32 is the bound's factor (the convention of field_maths_reference.compare)."""
    ld_dy, ld_x = ld_dy or n_out, ld_x or k_in
    g = torch.Generator().manual_seed(1000 * n_out + k_in + seed)
    dy, x = torch.randn(n_pts, ld_dy, generator=g), torch.randn(n_pts, ld_x, generator=g)
    a, b = dy[:, :n_out], x[:, :k_in]
    if rounded:
        a, b = a.bfloat16().float(), b.bfloat16().float()
    ref, S = a.double().t() @ b.double(), a.abs().double().t() @ b.abs().double()
    acc = torch.zeros(n_out, k_in, dtype=f32)
    for m0 in range(0, n_pts, 16):
        acc = acc + a[m0:m0 + 16].t() @ b[m0:m0 + 16]
    ratio32 = float(((acc.double() - ref).abs() / (ULP * S)).max())
    return {"dy": dy, "x": x, "ref": ref, "S": S, "ratio32": ratio32, "K": 4.0 * ratio32}


# ---------------------------------------------------------------------------------------------- the cases of the GPU file
SEG_LENS = (528, 0, 37, 1203, 3)  # an empty segment, one below a stage, boundaries off the stage (vprefix shifts the deal)
# n_out, k_in, ld_dy, ld_x, elements the X rows start off their (aligned) allocation
VARIANT_SHAPES = (
    (64, 64, 64, 64, 0), (128, 104, 128, 104, 0), (256, 256, 256, 256, 0),      # vector X and dY: NKB 2, 4, 8 with P 1, 2, 4
    (256, 128, 256, 128, 0), (64, 256, 64, 256, 0), (128, 64, 128, 64, 0),      # ... the other pairings of NKB and P
    (16, 256, 16, 256, 0), (3, 128, 4, 128, 0), (16, 64, 16, 64, 0),            # <= 32 outputs: vector X, scalar dY, one row block
    (200, 104, 201, 104, 0),                                                    # vector X, scalar dY, P = 4, a last wave with one live block
    (128, 40, 128, 40, 0),                                                      # vector loads with clamped lanes: 40 of NKB 2's 64 columns
    (250, 99, 251, 99, 0), (37, 130, 38, 132, 0), (40, 50, 41, 51, 0),          # scalar loads: NKB 4, 8, 2
    (256, 256, 256, 256, 1), (64, 64, 64, 64, 1))                               # an aligned shape with X 4 bytes off: scalar loads
STAGE_SHAPES = ((64, 64), (128, 104), (256, 256))  # NKB 2, 4, 8 of the split-bf16 kernel
TAIL_POINTS = 15
COUNT_SHAPES = ((64, 64, 64, 64), (128, 104, 128, 104), (256, 256, 256, 256), (16, 256, 16, 256), (250, 99, 251, 99))
EIGHT_LENS = (160, 7, 333, 16, 1, 640, 77, 256)
EIGHT_COUNTS = {2: (50, 5), 5: (0, 64), 7: (9, 64)}  # segment: (device count, rows per count): 250 of 333, 0 of 640, 576 -> 256 of 256
JOB_LENS = (300, 0, 33, 200)
MAP_WIDTH = 120
# n_out, k_in, ld_dy, X rows bf16, dY rows bf16
BF16_ROW_SHAPES = ((256, 256, 256, True, True), (128, 104, 128, True, True), (64, 64, 64, True, True), (37, 64, 38, True, True),
                   (256, 256, 256, False, True), (256, 104, 256, False, True), (128, 40, 128, False, True),
                   (16, 256, 16, True, False), (3, 128, 4, True, False), (16, 64, 16, True, False))
# mode, n_out, k_in, ld_dy, ld_x of the random cases: one per mode and variant family
RANDOM_CASES = (("f32", 256, 256, 256, 256), ("f32", 64, 64, 64, 64), ("f32", 16, 256, 16, 256), ("f32", 250, 99, 251, 99),
                ("bf16x6", 64, 64, 64, 64), ("bf16x6", 128, 104, 128, 104), ("bf16x6", 256, 256, 256, 256),
                ("bf16", 256, 256, 256, 256), ("bf16", 128, 104, 128, 104), ("bf16", 3, 128, 4, 128))


def shape_id(s):
    return "%dx%d-ld%d.%d%s" % (s[0], s[1], s[2], s[3], "-x+4" if s[4] else "")


def live_rows(lens, counts):
    """Indices of the points a call reads when segment s holds min(lens[s], count * rows per count) rows."""
    out, m0 = [], 0
    for s, n in enumerate(lens):
        live = min(n, counts[s][0] * counts[s][1]) if s in counts else n
        out.append(torch.arange(m0, m0 + live))
        m0 += n
    return torch.cat(out)


def column_map(k_in, width):
    """Packed column k -> destination column: a permutation into `width` columns (37 is coprime to it), every 13th dropped."""
    assert math.gcd(37, width) == 1 and width >= k_in
    return [-1 if k % 13 == 5 else (37 * k + 11) % width for k in range(k_in)]


def modelled_grid(lens, n_out, k_in, cus, products=6):
    """wgrad_grid of rsn_wgrad.hip restated for a split-bf16 launch of one job (16-point stages): what tests/test_wgrad_exact_cpu.py
    searches segment lengths against, for several CU counts.  The GPU file asks the library itself."""
    nkb, nsub = nkb_of(k_in), nsub_of(n_out)
    stages = sum((n + 15) // 16 for n in lens)
    t_stage = (2 if n_out > 32 else 1) * nkb * 32 / 1.9e9 * products
    t_flush = n_out * k_in * 4.0 / 1.3e12 + 2e-8
    return max(1, min(int(math.sqrt(stages * t_stage / (nsub * t_flush)) + 0.5), cus))
