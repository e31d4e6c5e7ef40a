"""CPU: why the ragged first-layer dx (speechseparation_amd/csrc/critic_grad.hip, critic_dx_h2_kernel<true>) forms its scale exponent
per CLIP.  The scheme of tests/test_critic_grad_reference.py (its `emulate`, float32 numpy) is evaluated on two clips of a batch, the
second one's dp1 a power of two smaller than the first's, once with one exponent for the batch (e = 14 - floor(log2 max |dp1|) over both
clips: what a loop-free reuse of the per-call rule would do) and once with the clip's own, and held to `dx_bound` of the clip ALONE (its
m is the clip's own maximum), against float64 on the clip alone.

What it shows (worst error / bound over the small clip's elements, 2 channels, 601 frames):

    ratio of the maxima     one exponent per batch     the clip's own exponent
    2^-20                   0.0002                     0.0003
    2^-32                   0.007                      0.0002
    2^-40                   1.8                        0.0003
    2^-44                   47                         0.0002

At 2^-20 the batch's exponent still meets the bound: the scaled small clip lies around 2^-8, inside fp16's normal range, and both pieces
keep their 22 bits.  The loss sets in once the scaled values fall below fp16's subnormal grid of 2^-24 (from about 2^-36 on): the first
piece is zero and the second keeps a few bits.  So the GPU test carries both a 2^-20 clip and a 2^-44 clip; only the second separates
the two rules.  (A score's dp1 scales with gscale[c] * s_c (1 - s_c) / (rows_c T4_c): a saturated clip or a zero-weighted one beside an
ordinary one reaches such ratios.)"""
import numpy as np
import pytest

import test_critic_grad_reference as gr


def _two_clips(k, seed=11, I=2, T=601):
    rng = np.random.default_rng(seed)
    w = gr.weights(rng, I)
    dp = (1e-8 * rng.standard_normal((2, gr.O, gr.frames_out(T)))).astype(np.float32)
    dp[1] *= np.float32(2.0 ** -k)
    return w, dp, T


@pytest.mark.parametrize("k", [20, 44])
def test_one_exponent_per_batch_against_the_clips_own(k):
    w, dp, T = _two_clips(k)
    small = dp[1:2]
    per_batch = gr.worst_ratio(gr.emulate(w, dp, T)[1:2], w, small, T)           # e from the maximum over both clips
    per_clip = gr.worst_ratio(gr.emulate(w, small, T), w, small, T)              # e from the clip's own maximum
    big = gr.worst_ratio(gr.emulate(w, dp, T)[0:1], w, dp[0:1], T)               # (the large clip is served by either)
    print("maxima 2^-%d apart: worst error / bound of the small clip, one exponent per batch %.4g, the clip's own %.4g" % (k, per_batch, per_clip))
    assert per_clip <= 1.0 and big <= 1.0
    if k == 20:
        assert per_batch <= 1.0                                                  # still inside fp16's normal range: no loss yet
    else:
        assert per_batch > 10.0                                                  # misses the clip's bound by more than an order of magnitude


def test_the_small_clips_exponent_is_its_own():
    """The exponent of a clip is a function of its own maximum: 14 - floor(log2 max), whatever stands beside it."""
    w, dp, _ = _two_clips(44)
    assert gr.scale_exponent(dp) == gr.scale_exponent(dp[0:1])                   # the batch's is the large clip's
    assert abs(gr.scale_exponent(dp[1:2]) - gr.scale_exponent(dp) - 44) <= 1     # (two draws: the maxima's ratio is 2^-44 up to a factor of 2)
