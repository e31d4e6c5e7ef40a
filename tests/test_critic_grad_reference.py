"""CPU: the scaled three-term fp16x2 scheme of the committed critic's first-layer dx (speechseparation_amd/csrc/critic_grad.hip), evaluated
in float32 numpy, against float64 - the bound the GPU test holds the kernel to is derived here, is not vacuous, and the scheme meets it.

The product (critic_grad_host.h): G[(i, k)][t] = sum_o W[o][i][k] dp[c][o][t] over K = o = 1024, then dx[c][i][s] = the sum over the taps
k = s % 3, s % 3 + 3, ... of G[(i, k)][(s - k) / 3], in tap order.

The emulation: e = 14 - floor(log2 max |dp|) over the whole call, dp' = dp 2^e (exact); both operands split as gemm.hip's Piece<2> does
(a1 = fp16(a), a2 = fp16(2^11 (a - a1)), round to nearest even, fp16 subnormals kept), products of two fp16 values exact, one matrix
instruction = the sum over its K step of 16 output channels added to an fp32 accumulator with one rounding, lo += a2 b1, lo += a1 b2,
hi += a1 b1, G = fl(hi + fl(2^-11 lo)), the fold in fp32 in tap order, the result times 2^-e (exact).

THE BOUND, per element, with n = 1024 x (the element's taps) products, u = 2^-24, S = sum |W| |dp| over them, m = max |dp| of the call:

    (n + 14) u S  +  2^-49 m sum |W|  +  2^-35 sum |dp|  +  2^-64 m n

(n + 2) u S is the fp32 sum's (tests/critic_reference.py, bound; the scheme rounds far less often than once per product).  12 u S is what
the operands' representation costs where every first piece is a NORMAL fp16 number (tests/test_critic_score_reference.py): 22 significant
bits per operand and the dropped term a2 b2, 3 x 2^-22 per product.  The other three terms are what operands whose first piece falls into
fp16's subnormals cost.  There both pieces round on the fixed grid 2^-24: the first leaves a remainder of at most 2^-25, the second
represents 2^11 times it to within 2^-25, so such an operand is off by at most 2^-36 ABSOLUTE, and the part its second piece carries is at
most 2^-25 (not 2^-11 of the operand).  Per product a b, a = W, b = dp', with |da| <= 2^-22 |a| + 2^-36, |db| <= 2^-22 |b| + 2^-36 and
second pieces' values at most 2^-11 |a| + 2^-25, 2^-11 |b| + 2^-25:
    |a b - (a1 b1 + 2^-11 (a1 b2 + a2 b1))| <= |da| |b| + |a| |db| + (2^-11 |a| + 2^-25)(2^-11 |b| + 2^-25)
                                            <= 3 x 2^-22 |a b| + 2 x 2^-36 |b| + 2 x 2^-36 |a| + 2^-50
In dp's own units (times 2^-e, and 2^-e <= 2^-14 m because the scaled maximum is at least 2^14): 2^-35 |dp| for the weights' side, which
no scaling helps (the issue's proposal leaves it out: a weight below 2^-14 keeps fewer than 22 bits), 2^-49 m |W| for dp's side (the
proposal has 2^-50: it counts the representation but not the dropped term's share), and 2^-64 m.  With weights around 2^-8 the three are
below a hundredth of the first term; they are kept because they are what the arithmetic gives.

Without the scale the bound is missed by orders of magnitude on a realistic dp (1e-8: below fp16's smallest subnormal, the first piece is
zero and the second keeps a few bits), which the last test shows."""
import numpy as np
import pytest

U = 2.0 ** -24
O, TAPS, STRIDE = 1024, 16, 3


def frames_out(T):
    return (T - TAPS) // STRIDE + 1


def split(a):
    a = a.astype(np.float32)
    a1 = a.astype(np.float16).astype(np.float32)
    a2 = ((a - a1) * np.float32(2048)).astype(np.float16).astype(np.float32)
    return a1, a2


def fold(G, T, dtype):
    """G [C, I, 16, T1] -> [C, I, T]: position s takes tap k from frame (s - k) / 3, taps added in tap order; zeros where no window reaches."""
    C, I, _, T1 = G.shape
    out = np.zeros((C, I, T), dtype)
    for k in range(TAPS):
        out[:, :, k:k + STRIDE * T1:STRIDE] += G[:, :, k, :]
    return out


def product(w, d):
    """[1024, I, 16] x [C, 1024, T1] -> [C, I, 16, T1], summed over the output channels."""
    return np.tensordot(w, d, axes=([0], [1])).transpose(2, 0, 1, 3)


def dx_float64(w, dp, T):
    """The definition in float64: w [1024, I, 16], dp [C, 1024, T1] -> dx [C, I, T]."""
    return fold(product(w.astype(np.float64), dp.astype(np.float64)), T, np.float64)


def dx_bound(w, dp, T):
    """The bound above for every element of dx [C, I, T]."""
    w64, d64 = np.abs(w.astype(np.float64)), np.abs(dp.astype(np.float64))
    C, _, T1 = dp.shape
    I = w.shape[1]
    S = fold(product(w64, d64), T, np.float64)
    taps = fold(np.ones((C, I, TAPS, T1)), T, np.float64)
    sum_w = fold(np.broadcast_to(w64.sum(axis=0)[None, :, :, None], (C, I, TAPS, T1)), T, np.float64)
    sum_d = fold(np.broadcast_to(d64.sum(axis=1)[:, None, None, :], (C, I, TAPS, T1)), T, np.float64)
    m = float(d64.max())
    n = O * taps
    return (n + 14) * U * S + 2.0 ** -49 * m * sum_w + 2.0 ** -35 * sum_d + 2.0 ** -64 * m * n


def scale_exponent(dp):
    m = float(np.abs(dp.astype(np.float32)).max())
    return 0 if m == 0.0 or not np.isfinite(m) else 14 - int(np.floor(np.log2(m)))


def emulate(w, dp, T, scaled=True, kstep=16):
    """w [1024, I, 16], dp [C, 1024, T1] float32 -> dx [C, I, T] float32 by the scheme above (scaled=False: the plain split of dp)."""
    C, _, T1 = dp.shape
    I = w.shape[1]
    e = scale_exponent(dp) if scaled else 0
    a1, a2 = split(w)
    b1, b2 = split(np.ldexp(dp.astype(np.float32), e))
    A = [p.reshape(O, I * TAPS).T.astype(np.float64) for p in (a1, a2)]          # [(i, k), o]
    G = np.empty((C, I, TAPS, T1), np.float32)
    for c in range(C):
        B = [p[c].astype(np.float64) for p in (b1, b2)]                          # [o, t]
        hi = np.zeros((I * TAPS, T1), np.float32)
        lo = np.zeros((I * TAPS, T1), np.float32)
        for k in range(0, O, kstep):
            s = slice(k, k + kstep)
            lo = (lo + A[1][:, s] @ B[0][s]).astype(np.float32)
            lo = (lo + A[0][:, s] @ B[1][s]).astype(np.float32)
            hi = (hi + A[0][:, s] @ B[0][s]).astype(np.float32)
        G[c] = (hi + lo * np.float32(1.0 / 2048)).reshape(I, TAPS, T1)
    return np.ldexp(fold(G, T, np.float32), -e)


def weights(rng, I):
    return rng.uniform(-0.0039, 0.0039, (O, I, TAPS)).astype(np.float32)


def small_dp(rng, C, T1):
    """A realistic dp1: 1e-8 N(0, 1), every row after the first 2^-20 times smaller than the first."""
    dp = (1e-8 * rng.standard_normal((C, O, T1))).astype(np.float32)
    dp[1:] *= np.float32(2.0 ** -20)
    return dp


def worst_ratio(got, w, dp, T):
    # (a position no window reaches has bound 0 and must be exactly 0)
    return float((np.abs(got.astype(np.float64) - dx_float64(w, dp, T)) / np.maximum(dx_bound(w, dp, T), np.finfo(np.float64).tiny)).max())


def test_fold_is_the_definition():
    rng = np.random.default_rng(5)
    T, I = 603, 2
    T1 = frames_out(T)
    w, dp = weights(rng, I), rng.standard_normal((1, O, T1)).astype(np.float32)
    ref = np.zeros((1, I, T))
    w64, d64 = w.astype(np.float64), dp.astype(np.float64)
    for s in range(T):
        for k in range(TAPS):
            if s - k >= 0 and (s - k) % STRIDE == 0 and (s - k) // STRIDE < T1:
                ref[0, :, s] += w64[:, :, k].T @ d64[0, :, (s - k) // STRIDE]
    got = dx_float64(w, dp, T)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    assert (got[:, :, STRIDE * (T1 - 1) + TAPS:] == 0).all() and T - (STRIDE * (T1 - 1) + TAPS) == 2      # the two trailing positions of 603


@pytest.mark.parametrize("kstep", [16, 32])
@pytest.mark.parametrize("case", ["normal", "normal-1e-6", "small-two-rows"])
@pytest.mark.parametrize("shape", [(2, 601), (10, 793), (66, 601)], ids=lambda s: "%d-%d" % s)
def test_scaled_three_term_scheme_within_the_bound(shape, case, kstep):
    I, T = shape
    rng = np.random.default_rng(200 + I)
    T1 = frames_out(T)
    w = weights(rng, I)
    if case == "small-two-rows":
        dp = small_dp(rng, 2, T1)
    else:
        dp = (rng.standard_normal((1, O, T1)) * (1.0 if case == "normal" else 1e-6)).astype(np.float32)
    ratio = worst_ratio(emulate(w, dp, T, kstep=kstep), w, dp, T)
    print("I = %d, T = %d, %s, K step %d: worst error / bound = %.4f" % (I, T, case, kstep, ratio))
    assert ratio <= 1.0


def test_integers_are_exact():
    rng = np.random.default_rng(7)
    I, T = 7, 602
    w = rng.integers(-2, 3, (O, I, TAPS)).astype(np.float32)
    dp = rng.integers(-2, 3, (3, O, frames_out(T))).astype(np.float32)
    assert (emulate(w, dp, T).astype(np.float64) == dx_float64(w, dp, T)).all()


def test_without_the_scale_a_small_dp_misses_the_bound():
    rng = np.random.default_rng(11)
    I, T = 2, 601
    w, dp = weights(rng, I), small_dp(rng, 2, frames_out(T))
    with_scale = worst_ratio(emulate(w, dp, T), w, dp, T)
    without = worst_ratio(emulate(w, dp, T, scaled=False), w, dp, T)
    print("dp ~ 1e-8: worst error / bound with the scale %.4f, without %.1f" % (with_scale, without))
    assert with_scale <= 1.0 and without > 100.0


def second_piece_case(rng, I, C, T):
    """Operands that need the second piece and still give exact fp32 sums: W = a + b 2^-12 with a, b in {-1, 0, 1} (first piece a, second
    piece b / 2), dp in {-1, 0, 1}.  Every partial sum is a multiple of 2^-12 below 2^12 in magnitude for these draws (checked)."""
    w = (rng.integers(-1, 2, (O, I, TAPS)) + rng.integers(-1, 2, (O, I, TAPS)) * 2.0 ** -12).astype(np.float32)
    dp = rng.integers(-1, 2, (C, O, frames_out(T))).astype(np.float32)
    assert float(fold(product(np.abs(w.astype(np.float64)), np.abs(dp.astype(np.float64))), T, np.float64).max()) < 2.0 ** 13
    return w, dp


def test_what_catches_a_lost_second_piece():
    """The bound grows with n >= 5120 products per element and random errors with sqrt(n): a product of the FIRST pieces alone stays
    inside it on normal variates (printed; about 0.4).  What the bound excludes is a wrong scale (above) and anything structural; a lost
    or misplaced second piece is caught by operands whose second pieces matter and whose sums are exact: there the scheme equals
    float64 bit for bit and the first pieces alone do not."""
    rng = np.random.default_rng(13)
    I, T = 2, 601
    T1 = frames_out(T)
    w, dp = weights(rng, I), rng.standard_normal((1, O, T1)).astype(np.float32)
    plain = fold(product(split(w)[0].astype(np.float64), split(dp)[0].astype(np.float64)), T, np.float64)
    print("first pieces alone on normal variates: worst error / bound = %.3f" % worst_ratio(plain, w, dp, T))
    w, dp = second_piece_case(rng, 7, 2, 602)
    ref = dx_float64(w, dp, 602)
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()             # representable: nothing to round
    assert (emulate(w, dp, 602).astype(np.float64) == ref).all()
    first = fold(product(split(w)[0].astype(np.float64), dp.astype(np.float64)), 602, np.float64)
    assert (first != ref).mean() > 0.5


def test_extra_terms_are_small_beside_the_first():
    rng = np.random.default_rng(17)
    I, T = 10, 601
    w, dp = weights(rng, I), small_dp(rng, 2, frames_out(T))
    b = dx_bound(w, dp, T)[0]                                                    # the large row (the small one lives on the m sum |W| term)
    S = fold(product(np.abs(w.astype(np.float64)), np.abs(dp.astype(np.float64))), T, np.float64)[0]
    taps = fold(np.ones((1, I, TAPS, frames_out(T))), T, np.float64)[0]
    reach = taps > 0
    first = ((O * taps + 14) * U * S)[reach]
    assert float((b[reach] / first).max()) < 1.02
