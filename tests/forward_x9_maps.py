"""The two index maps of the training forward's trunk on the 16x16x32 shape (rsn_epilogues.h: init_acc16, store_act16_relu), stated
once in Python beside the maps of the fp32 loop they must agree with (store_act, ReluBits).  No GPU, no library.

The wave's output tile is 32 points x 32 NB rows.  A slab entry is (K-iteration it, old lane, component c): store_act writes
register 4 q + j of block nb of lane l to (4 nb + q, l, j), which is row 32 nb + 8 q + 4 (l >> 5) + j of point l & 31."""


def slab_entry32(lane, nb, q, j):
    """store_act: (it, old lane, component) of register 4 q + j of block nb of `lane`."""
    return 4 * nb + q, lane, j


def row_point32(lane, nb, q, j):
    """the unit (row) and the point of the tile behind that register (init_acc: bias[32 nb + 8 q + 4 h + j])"""
    return 32 * nb + 8 * q + 4 * (lane >> 5) + j, lane & 31


def row_point16(lane, nb, rh, ph, r):
    """16-shape: register r of result (nb, rh, ph) of `lane` is row 32 nb + 16 rh + 4 (L >> 4) + r of point (L & 15) + 16 ph"""
    return 32 * nb + 16 * rh + 4 * (lane >> 4) + r, (lane & 15) + 16 * ph


def slab_entry16(lane, nb, rh, ph, r):
    """store_act16 / store_act16_relu: one float4, K-iteration 4 nb + 2 rh + (L >> 5) of old lane (L & 15) + 16 ph + 32 ((L >> 4) & 1)"""
    return 4 * nb + 2 * rh + (lane >> 5), (lane & 15) + 16 * ph + 32 * ((lane >> 4) & 1), r


def bit32(lane, nb, q, j):
    """ReluBits: (old lane, word, bit) of register 4 q + j of block nb of `lane` (store_act: bit 16 (nb & 1) + 4 q + j of word nb / 2)"""
    return lane, nb // 2, 16 * (nb & 1) + 4 * q + j


def nibble16(lane, nb, rh, ph):
    """store_act16_relu: (old lane, word, first bit) of the nibble of result (nb, rh, ph) of `lane`"""
    return (lane & 15) + 16 * ph + 32 * ((lane >> 4) & 1), nb // 2, 16 * (nb & 1) + 4 * (2 * rh + (lane >> 5))


def storing_lane16(old_lane):
    """the lane that stores the mask words of `old_lane` behind the 32-lane exchange: point half kh = L >> 5, half (L >> 4) & 1"""
    m, h = old_lane & 31, old_lane >> 5
    return (m & 15) + 16 * h + 32 * (m >> 4)


def decode_relu_bits(words, width):
    """saved.relu_bits of one layer, int32 [n, 2, nw] (torch) -> bool [n, width]: unit 32 nb + 8 q + 4 h + j is bit
    16 (nb & 1) + 4 q + j of word nb / 2 of half h"""
    import torch

    n = words.shape[0]
    out = torch.zeros(n, width, dtype=torch.bool)
    w = words.to(torch.int64) & 0xFFFFFFFF
    for nb in range(width // 32):
        for q in range(4):
            for h in range(2):
                for j in range(4):
                    out[:, 32 * nb + 8 * q + 4 * h + j] = ((w[:, h, nb // 2] >> (16 * (nb & 1) + 4 * q + j)) & 1).bool()
    return out
