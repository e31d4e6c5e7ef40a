"""CPU: the three-term fp16x2 scheme of the committed critic's first layer (speechseparation_amd/csrc/critic_score.hip), evaluated in
float32 numpy, against float64 - the bound the GPU test holds the kernel to is not vacuous and the scheme itself meets it.

The emulation: both operands split as gemm.hip's Piece<2> does (a1 = fp16(a), a2 = fp16(2^11 (a - a1)), round to nearest even, fp16
subnormals kept), products of two fp16 values exact, one matrix instruction = the sum over its K step added to an fp32 accumulator with
one rounding, hi += a1 b1, lo += a2 b1, lo += a1 b2, a slab's value fl(hi + fl(2^-11 lo)), slabs added in order, then the bias.  K steps
of 16 (one input channel: v_mfma_f32_32x32x16_f16, the instruction the kernel uses) and of 32 (v_mfma_f32_16x16x32_f16).

The bound, per element: (n + 14) u S with n = 16 I products, u = 2^-24, S = sum |w| |x| + |b|.  (n + 2) u S is the fp32 dot product's
(tests/critic_reference.py, bound).  The 12 u S more is what the operands' representation costs: a ~ a1 + 2^-11 a2 keeps 22 significant
bits, |a - (a1 + 2^-11 a2)| <= 2^-22 |a| (the second piece's rounding, 2^-11 of a remainder of at most 2^-11 |a|), so a product of two
such operands is off by 2 x 2^-22 relative, and the dropped term a2 b2 2^-22 is at most (2^-11)^2 |a| |b| = 2^-22 |a b|: 3 x 2^-22 =
12 u per product, summed over the products: 12 u S.  Weights below 2^-14 (about 1.5 % of uniform +-0.0039) have a subnormal first piece;
their second piece takes up what the first loses, which is what the scaling by 2^11 is for."""
import numpy as np
import pytest

U = 2.0 ** -24
F16_MIN_NORMAL = 2.0 ** -14


def split(a):
    a = a.astype(np.float32)
    a1 = a.astype(np.float16).astype(np.float32)
    a2 = ((a - a1) * np.float32(2048)).astype(np.float16).astype(np.float32)
    return a1, a2


def emulate(x, w, b, kstep, ch_per_slab):
    """x [I, T], w [O, I, 16], b [O] float32 -> pre-activation [O, T1] float32 by the scheme above."""
    I, T = x.shape
    O = w.shape[0]
    T1 = (T - 16) // 3 + 1
    xw = np.stack([x[:, 3 * t:3 * t + 16] for t in range(T1)], axis=1)           # [I, T1, 16]
    a1, a2 = split(w)
    b1, b2 = split(xw)
    A = [p.reshape(O, I * 16).astype(np.float64) for p in (a1, a2)]
    B = [p.transpose(0, 2, 1).reshape(I * 16, T1).astype(np.float64) for p in (b1, b2)]
    total = None
    for lo_ch in range(0, I, ch_per_slab):
        k_lo, k_hi = 16 * lo_ch, 16 * min(I, lo_ch + ch_per_slab)
        hi = np.zeros((O, T1), np.float32)
        lo = np.zeros((O, T1), np.float32)
        for k in range(k_lo, k_hi, kstep):
            s = slice(k, min(k + kstep, k_hi))
            lo = (lo + A[1][:, s] @ B[0][s]).astype(np.float32)
            lo = (lo + A[0][:, s] @ B[1][s]).astype(np.float32)
            hi = (hi + A[0][:, s] @ B[0][s]).astype(np.float32)
        part = hi + lo * np.float32(1.0 / 2048)
        total = part if total is None else total + part
    return total + b[:, None]


@pytest.mark.parametrize("kstep", [16, 32])
@pytest.mark.parametrize("scale", [1.0, 1e-4], ids=["normal", "normal-1e-4"])
@pytest.mark.parametrize("I", [1, 2, 66])
def test_three_term_scheme_within_the_bound(I, scale, kstep):
    rng = np.random.default_rng(100 + I)
    O, T = 1024, 601
    w = rng.uniform(-0.0039, 0.0039, (O, I, 16)).astype(np.float32)
    b = rng.uniform(-0.0039, 0.0039, (O,)).astype(np.float32)
    x = (rng.standard_normal((I, T)) * scale).astype(np.float32)
    small = float((np.abs(w) < F16_MIN_NORMAL).mean())
    assert 0.005 < small < 0.03, small                                           # the subnormal first pieces are there
    got = emulate(x, w, b, kstep, ch_per_slab=10).astype(np.float64)
    T1 = (T - 16) // 3 + 1
    xw = np.stack([x[:, 3 * t:3 * t + 16] for t in range(T1)], axis=1).astype(np.float64)
    w64 = w.astype(np.float64)
    ref = np.einsum("oik,itk->ot", w64, xw) + b[:, None]
    S = np.einsum("oik,itk->ot", np.abs(w64), np.abs(xw)) + np.abs(b)[:, None]
    n = 16 * I
    ratio = float((np.abs(got - ref) / ((n + 14) * U * S)).max())
    print("I = %d, x scale %g, K step %d: worst error / ((n + 14) u S) = %.3f   (over (n + 2) u S: %.3f)" % (
        I, scale, kstep, ratio, ratio * (n + 14) / (n + 2)))
    assert ratio <= 1.0
    # not vacuous: one fp16 piece per operand (a1 b1 alone) misses the bound several times over where few products meet (the bound grows
    # with n, random errors with sqrt(n): at 66 channels even plain fp16 stays inside it, which is why the narrow layers are the test)
    if I > 2:
        return
    a1, _ = split(w)
    b1, _ = split(xw)
    plain = np.einsum("oik,itk->ot", a1.astype(np.float64), b1.astype(np.float64)) + b[:, None]
    assert float((np.abs(plain - ref) / ((n + 14) * U * S)).max()) > 5.0
