"""A host model of the piece-product K loops (rsn_gemm_loops.h, mma16s): six of the nine products of three bf16 pieces a side against
all nine, and both against the sequential fp32 MFMA loop.

Operands are split as split8<3> splits them (three round-to-nearest-even bf16 pieces); per K = 32 step the products of one piece
pair are summed without rounding (fp64 holds them: 16-bit products, 32 of them, a narrow exponent range) and each such sum is added
to an fp32 accumulator, smallest pair first, as one MFMA adds it.  The fp32 loop adds two exact products per MFMA (K = 2) to its fp32
accumulator.  That is not the hardware's internal summation, which is not documented to the bit: the model says what dropping the
three smallest products costs against the rounding of the accumulation itself, nothing more.

Weights uniform in +-1/16, activations log-normal with half of them zero (a masked gradient row), fixed seed."""
import numpy as np
import pytest

PROD_W = (2, 2, 1, 2, 1, 0, 1, 0, 0)  # prod_wp / prod_bp of rsn_gemm_loops.h: 0 = hi, 1 = mid, 2 = lo
PROD_B = (2, 1, 2, 0, 1, 2, 0, 1, 0)


def bf16_rne(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    hi = bf16_rne(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_rne(r1)
    lo = bf16_rne((r1 - mid).astype(np.float32))
    return hi, mid, lo


def piece_sum(w, b, n_products):
    """[N, K] fp32 operands -> [N] fp32: the last n_products of the nine piece products per K = 32 step, in the loop's order."""
    wp, bp = split3(w), split3(b)
    acc = np.zeros(w.shape[0], np.float32)
    for s in range(0, w.shape[1], 32):
        for p in range(9 - n_products, 9):
            step = (wp[PROD_W[p]][:, s:s + 32].astype(np.float64) * bp[PROD_B[p]][:, s:s + 32].astype(np.float64)).sum(axis=1)
            acc = (acc.astype(np.float64) + step).astype(np.float32)
    return acc


def fp32_loop(w, b):
    acc = np.zeros(w.shape[0], np.float32)
    for k in range(0, w.shape[1], 2):
        step = (w[:, k:k + 2].astype(np.float64) * b[:, k:k + 2].astype(np.float64)).sum(axis=1)
        acc = (acc.astype(np.float64) + step).astype(np.float32)
    return acc


def operands(n, k, seed):
    g = np.random.default_rng(seed)
    w = g.uniform(-1.0 / 16, 1.0 / 16, (n, k)).astype(np.float32)
    b = (np.exp(g.normal(0.0, 1.0, (n, k))) * np.sign(g.normal(size=(n, k))) * (g.random((n, k)) < 0.5)).astype(np.float32)
    return w, b


@pytest.mark.parametrize("k", [64, 256])
def test_six_products_cost_nothing_against_the_accumulations_rounding(k):
    w, b = operands(20000, k, seed=k)
    ref = (w.astype(np.float64) * b.astype(np.float64)).sum(axis=1)
    err = {name: np.abs(v.astype(np.float64) - ref) for name, v in
           (("nine", piece_sum(w, b, 9)), ("six", piece_sum(w, b, 6)), ("fp32", fp32_loop(w, b)))}
    worst = {n: float(e.max()) for n, e in err.items()}
    rms = {n: float(np.sqrt((e ** 2).mean())) for n, e in err.items()}
    print(f"K = {k}: worst / RMS error against fp64: nine {worst['nine']:.3e} / {rms['nine']:.3e}, six {worst['six']:.3e} / {rms['six']:.3e}, "
          f"fp32 loop {worst['fp32']:.3e} / {rms['fp32']:.3e}; six over nine {worst['six'] / worst['nine']:.3f} / {rms['six'] / rms['nine']:.3f}")
    assert worst["six"] <= 1.05 * worst["nine"]
    assert rms["six"] <= 1.05 * rms["nine"]
    assert worst["nine"] < worst["fp32"] and worst["six"] < worst["fp32"]
    assert rms["nine"] < rms["fp32"] and rms["six"] < rms["fp32"]


@pytest.mark.parametrize("which", ["weights", "activations"])
def test_an_operand_of_hi_pieces_alone_makes_six_equal_nine(which):
    w, b = operands(4000, 64, seed=7)
    if which == "weights":
        w = bf16_rne(w)
    else:
        b = bf16_rne(b)
    # every dropped product carries a mid or lo piece of BOTH operands or a lo piece of one and a mid / lo piece of the other: with
    # one operand all hi, each of the three has a zero factor and adds +-0 to the accumulator
    nine, six = piece_sum(w, b, 9), piece_sum(w, b, 6)
    assert np.array_equal(nine.view(np.uint32), six.view(np.uint32))
