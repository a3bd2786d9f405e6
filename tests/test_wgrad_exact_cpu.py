"""The integer cases of tests/test_wgrad_exact_gpu.py are meaningful (no GPU, no library call): for every class and shape of that
file the host asserts what makes the case exact (tests/wgrad_cases.Case.assert_meaningful), the restatement of split2 and mma6
returns the fp64 reference exactly, and each way the kernel could be subtly wrong gives ANOTHER integer matrix:

  * one kept product removed: more than half of the entries of the class built for it change (A: lo x hi, B: hi x lo, C: mid x mid),
    and every product that carries a class changes it;
  * a3 paired with b2 instead of b1 (and the mirror, and mid x mid replaced);
  * one point dropped; two rows or two columns of the result swapped.

It also recomputes the table of DESIGN 4.24 on random operands and asserts it as what it is: the removal of each SMALL product
stays UNDER the suite's 2e-5 max|ref| bound -- the documented reason the integer cases exist.  The deal of stages to wave slots is
restated (wgrad_cases.slot_stages) and the search for full-stage segment lengths is run against the launcher's grid formula for
several CU counts."""
import pytest
import torch

from tests import wgrad_cases as W

N_SEG = sum(W.SEG_LENS)


def _shape_cases():
    """(class, points, n_out, k_in, ld_dy, ld_x) of every integer case of the GPU file whose lengths are fixed; the full-stage runs'
    lengths follow from the device's grid and are asserted there, on the host, before the launch (and below for modelled grids)."""
    out = []
    for n_out, k_in, ld_dy, ld_x, _ in W.VARIANT_SHAPES:
        out += [(cls, N_SEG, n_out, k_in, ld_dy, ld_x) for cls in W.CLASSES]
    for n_out, k_in in W.STAGE_SHAPES:
        out += [(cls, W.TAIL_POINTS, n_out, k_in, n_out, k_in) for cls in "ABC"]
    out += [(cls, N_SEG, 256, 104, 256, 104) for cls in "BD"]
    for n_out, k_in in ((256, 256), (128, 104), (64, 64)):
        out += [(cls, sum(W.JOB_LENS), n_out, k_in, n_out, k_in) for cls in "AB"]
    for n_out, k_in, ld_dy, _, _ in W.BF16_ROW_SHAPES:
        out.append(("D", N_SEG, n_out, k_in, ld_dy, k_in))
    return sorted(set(out))


SHAPE_CASES = _shape_cases()


@pytest.mark.parametrize("cls,n_pts,n_out,k_in,ld_dy,ld_x", SHAPE_CASES)
def test_case_is_exact_and_every_mutation_shows(cls, n_pts, n_out, k_in, ld_dy, ld_x):
    c = W.case(cls, n_pts, n_out, k_in, ld_dy, ld_x)
    c.assert_meaningful(want_db=cls != "A", label="cpu")
    assert cls != "A" or n_pts < 64 or not c.db_exact(), "class A is expected to break the bias bound: the GPU file passes db = NULL there"
    a, b = c.operands()
    ref, ref_b = c.reference()
    assert bool((ref == ref.round()).all()) and float(ref.abs().max()) < W.EXACT
    assert torch.equal(ref.float().double(), ref) and (cls == "A" or torch.equal(ref_b.float().double(), ref_b))
    assert torch.equal(W.six_products(a, b), ref), "the six-product restatement is not exact on this case"
    size = ref.numel()
    for p in W.KEPT:
        changed = int((W.six_products(a, b, W.without(p)) != ref).sum())
        if p in W.CARRIED_BY[cls]:
            assert changed > 0, f"removing {W.name(p)} does not show"
        else:
            assert changed == 0, f"{W.name(p)} is not expected to carry class {cls}"
        if W.BUILT_FOR.get(cls) == p:
            print(f"class {cls} {n_out}x{k_in}, {n_pts} points: without {W.name(p)} {changed} of {size} entries change")
            assert changed > size / 2, f"removing {W.name(p)} changes only {changed} of {size} entries"
    # a misplaced piece: a3 with b2 instead of b1, a1 with ... the mirror, mid x mid as mid x hi twice
    for cl, p, other in (("A", (2, 0), (2, 1)), ("B", (0, 2), (1, 2)), ("C", (1, 1), (1, 0))):
        if cls == cl:
            changed = int((W.six_products(a, b, W.swapped(p, other)) != ref).sum())
            assert changed > size / 2, f"{W.name(p)} swapped for {W.name(other)} changes only {changed} of {size} entries"
    # a dropped point (first, last, and around every boundary of the five segments)
    marks, m0 = {0, n_pts - 1}, 0
    for n in W.SEG_LENS if n_pts == N_SEG else ():
        marks |= {m0, m0 + n - 1} if n else set()
        m0 += n
    for m in sorted(marks):
        assert float(torch.outer(a[m].double(), b[m].double()).abs().max()) > 0, f"dropping point {m} does not show"
    # a permuted flush
    for i, j in ((0, 1), (0, n_out - 1), (n_out // 2, n_out // 2 - 1)):
        if i != j and min(i, j) >= 0:
            sw = ref.clone()
            sw[[i, j]] = ref[[j, i]]
            assert not torch.equal(sw, ref)
    for i, j in ((0, 1), (0, k_in - 1), (k_in // 2, k_in // 2 - 1)):
        sw = ref.clone()
        sw[:, [i, j]] = ref[:, [j, i]]
        assert not torch.equal(sw, ref)


@pytest.mark.parametrize("n_out,k_in,ld_dy,ld_x", W.COUNT_SHAPES)
def test_count_case_is_exact_on_its_live_rows(n_out, k_in, ld_dy, ld_x):
    rows = W.live_rows(W.EIGHT_LENS, W.EIGHT_COUNTS)
    assert rows.numel() == sum(W.EIGHT_LENS) - (333 - 250) - 640
    c = W.case("D", sum(W.EIGHT_LENS), n_out, k_in, ld_dy, ld_x)
    c.assert_meaningful(rows, want_db=True, label="counts")
    full, _ = c.reference()
    live, _ = c.reference(rows)
    assert int((full != live).sum()) > live.numel() / 2, "ignoring the device counts would not show"
    a, b = c.operands(rows)
    assert torch.equal(W.six_products(a, b), live)


def test_column_map_is_a_partial_permutation():
    cmap = W.column_map(104, W.MAP_WIDTH)
    kept = [c for c in cmap if c >= 0]
    assert len(set(kept)) == len(kept) and 0 < len(kept) < 104 and max(kept) < W.MAP_WIDTH
    assert kept != sorted(kept) and len(kept) < W.MAP_WIDTH  # it permutes, and some window columns are never reached


def test_pieces_are_the_kernels_split():
    """h + m + l == v exactly for integers below 2^24, each piece a bf16 value, nearest-even at the ties."""
    v = torch.tensor([257.0, 259.0, 2.0 ** 18 + 1, 2.0 ** 19 - 1, -(2.0 ** 18 + 2 ** 9 + 3), 1023.0, 15.0, 0.0])
    h, m, l = W.pieces(v)
    assert torch.equal(h + m + l, v)
    for p in (h, m, l):
        assert torch.equal(p.bfloat16().float(), p)
    assert float(h[0]) == 256.0 and float(h[1]) == 260.0  # bf16 steps by 2 here: both are ties and go to the even mantissa
    assert float(l[4]) != 0 and float(l[2]) == 0.0 and float(l[5]) == 0.0 and float(m[6]) == 0.0


# ---------------------------------------------------------------------------------------------- the deal of stages
@pytest.mark.parametrize("G", [1, 3, 37, 248])
def test_slot_stages_deal_every_stage_once(G):
    lens = list(W.SEG_LENS) + [16 * G + 5]
    for step in (8, 16):
        deal = W.slot_stages(lens, G, step)
        assert sum(c for row in deal for c, _ in row) == sum(n // step for n in lens)
        assert sum(t for row in deal for _, t in row) == sum(1 for n in lens if n % step)
        per_slot = [sum(c + t for c, t in row) for row in deal]
        assert max(per_slot) - min(per_slot) <= 1, "the round-robin deal is even to one stage"


@pytest.mark.parametrize("cus", [256, 304, 64, 8])
@pytest.mark.parametrize("n_out,k_in", W.STAGE_SHAPES)
def test_full_stage_search_covers_the_loop_shapes(n_out, k_in, cus):
    nsub = W.nsub_of(n_out)
    lens, G = W.full_stage_lengths(lambda ls: W.modelled_grid(ls, n_out, k_in, cus), nsub)
    seen, tails = W.counts_seen(lens, G, 16)
    assert seen == {0, 1, 2, 3, 4} and tails == 0 and all(n % 16 == 0 for n in lens)
    assert W.counts_seen([W.TAIL_POINTS], G, 16) == ({0}, 1)
    for cls in "ABC":
        c = W.case(cls, sum(lens), n_out, k_in)
        c.assert_meaningful(label=f"full stages, {cus} CUs")
        a, b = c.operands()
        ref, _ = c.reference()
        changed = int((W.six_products(a, b, W.without(W.BUILT_FOR[cls])) != ref).sum())
        assert torch.equal(W.six_products(a, b), ref) and changed > ref.numel() / 2


# ---------------------------------------------------------------------------------------------- why the integer cases exist
def test_random_operands_hide_a_dropped_small_product():
    """6043 randn points, 64 x 64 outputs, the six products in fp64 against the fp64 product: with nothing removed the error is a
    thousandth of the suite's bound 2e-5 max|ref|; with lo x hi, mid x mid or hi x lo removed it is STILL under the bound (a
    reduction on three products passes every random-operand test); only mid x hi or hi x mid leave it.  Entry by entry the same:
    a dropped small product moves no entry by more than 4 x 2^-24 S, the margin any float32 comparison needs."""
    g = torch.Generator().manual_seed(6043)
    a, b = torch.randn(6043, 64, generator=g), torch.randn(6043, 64, generator=g)
    ref, S = a.double().t() @ b.double(), a.abs().double().t() @ b.abs().double()
    bound = 2e-5 * float(ref.abs().max())
    err = lambda products: float((W.six_products(a, b, products) - ref).abs().max())  # noqa: E731
    rows = {"nothing": err(W.KEPT)}
    for p in W.KEPT[:5]:
        rows[W.name(p)] = err(W.without(p))
    for k, v in rows.items():
        print(f"removed {k:10s}: worst error {v:.2e}, {v / bound:.4f} of 2e-5 max|ref| = {bound:.2e}")
    assert rows["nothing"] < 1e-2 * bound
    for p in ((2, 0), (1, 1), (0, 2)):
        assert 10 * rows["nothing"] < rows[W.name(p)] < 0.5 * bound, f"{W.name(p)}: the existing bound was expected to hide its removal"
        moved = float(((W.six_products(a, b, W.without(p)) - ref).abs() / (W.ULP * S)).max())
        print(f"removed {W.name(p)}: worst entry moves by {moved:.2f} x 2^-24 S")
        assert moved < 4.0
    for p in ((1, 0), (0, 1)):
        assert rows[W.name(p)] > 10 * bound
    three = err(((1, 0), (0, 1), (0, 0)))
    print(f"three products only: {three:.2e}, {three / bound:.3f} of the bound")
    assert three < bound


@pytest.mark.parametrize("mode,n_out,k_in,ld_dy,ld_x", W.RANDOM_CASES)
def test_random_bound_factor_comes_from_the_float32_restatement(mode, n_out, k_in, ld_dy, ld_x):
    """K of the GPU file's entry-wise bound: 4 x the worst ratio of the float32 restatement, of the order of 1 x 2^-24 S."""
    r = W.random_case(6043, n_out, k_in, ld_dy, ld_x, rounded=False)
    print(f"{n_out}x{k_in}: float32 restatement worst ratio {r['ratio32']:.3f} -> K = {r['K']:.3f}")
    assert 0.25 < r["ratio32"] < 4.0 and r["K"] == 4.0 * r["ratio32"]
    assert float(r["S"].min()) > 0
