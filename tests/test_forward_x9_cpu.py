"""The index maps of the training forward's trunk on the 16x16x32 shape (tests/forward_x9_maps.py, the Python statement of
init_acc16 / store_act16_relu in rsn_epilogues.h) against the maps of the fp32 loop that everything behind the trunk reads by:
the slab layout of store_act and the ReluBits words.  Pure index arithmetic: no GPU, no library."""
import pytest

from tests import forward_x9_maps as M

NBS = (2, 4, 8)


@pytest.mark.parametrize("nb_count", NBS)
def test_output_map_is_a_bijection_onto_the_slab_layout(nb_count):
    """Over all 64 lanes and (nb, rh, ph, r): every slab entry of store_act is written once, and the unit and point behind it are
    the ones store_act puts there."""
    want = {}
    for lane in range(64):
        for nb in range(nb_count):
            for q in range(4):
                for j in range(4):
                    want[M.slab_entry32(lane, nb, q, j)] = M.row_point32(lane, nb, q, j)
    assert len(want) == 64 * nb_count * 16
    got = {}
    for lane in range(64):
        for nb in range(nb_count):
            for rh in range(2):
                for ph in range(2):
                    for r in range(4):
                        e = M.slab_entry16(lane, nb, rh, ph, r)
                        assert e not in got, f"slab entry {e} written twice"
                        got[e] = M.row_point16(lane, nb, rh, ph, r)
    assert got == want
    rows_points = sorted(got.values())
    assert rows_points == sorted((row, p) for row in range(32 * nb_count) for p in range(32))


@pytest.mark.parametrize("nb_count", NBS)
def test_nibble_map_is_a_bijection_onto_the_relu_bit_words(nb_count):
    """Every bit of the NB / 2 words of every old lane comes from one register of the 16-shape, the register of the same unit and
    point as the fp32 loop's; the two lanes that share a word hold alternate nibbles; one lane stores each old lane's words."""
    want = {}
    for lane in range(64):
        for nb in range(nb_count):
            for q in range(4):
                for j in range(4):
                    want[M.bit32(lane, nb, q, j)] = M.row_point32(lane, nb, q, j)
    assert len(want) == 64 * (nb_count // 2) * 32
    got, holders = {}, {}
    for lane in range(64):
        for nb in range(nb_count):
            for rh in range(2):
                for ph in range(2):
                    ol, word, b0 = M.nibble16(lane, nb, rh, ph)
                    assert b0 % 4 == 0 and (b0 // 4) % 2 == lane >> 5, "a lane's nibbles are those of its half K step"
                    holders.setdefault((ol, word), set()).add(lane)
                    for r in range(4):
                        key = (ol, word, b0 + r)
                        assert key not in got, f"bit {key} set twice"
                        got[key] = M.row_point16(lane, nb, rh, ph, r)
    assert got == want
    for (ol, _), lanes in holders.items():
        lo = min(lanes)
        assert lanes == {lo, lo ^ 32}, "the lanes that share a word are L and L ^ 32"
        assert M.storing_lane16(ol) in lanes
    assert sorted(M.storing_lane16(ol) for ol in range(64)) == list(range(64))


def test_decode_relu_bits_inverts_the_word_layout():
    import torch

    width = 128
    words = torch.zeros(1, 2, 2, dtype=torch.int32)
    unit = 32 * 3 + 8 * 2 + 4 * 1 + 3  # nb 3, q 2, h 1, j 3
    words[0, 1, 1] = 1 << (16 + 4 * 2 + 3)
    mask = M.decode_relu_bits(words, width)
    assert mask.sum() == 1 and bool(mask[0, unit])
