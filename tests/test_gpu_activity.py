"""GPU: the per-hop activity kernel (mining.hop_activity -> bsrnn_hop_activity) against tests/sections_reference.activity - the same fp32
terms in numpy, float64 sums.

Tolerance: finite values relative 1e-12.  Both sides add the same 1024 non-negative fp32 terms in double, in different orders; each sum
is off by at most 1023 * 2^-53 = 1.1e-13 of itself, so the two differ by at most 2.3e-13: the bound leaves a factor of four.  Inf, NaN
and exact 0 must match exactly, by position.  The inputs have |w| >= 2^-30 or are exactly 0 and |w - e| >= 0.2 |w|, so no square is
subnormal and flush-to-zero could not show (the library does not flush; the terms would differ if it did).

Shapes, the smallest that can go wrong: one hop of one row; three rows of 1, 2 and 5 hops in a rectangle of 5 (a partial hop group of
the kernel's four waves, rows that end early); no hop table; a hop count of 0; rows Hmax * 1024 + 3 floats apart from a base one float
off alignment (scalar loads) and the same aligned (16-byte loads), bit for bit; different strides for the two signals.  The only
comparisons of the library with itself are the equalities the interface promises (the two load paths, a row in a batch == the row alone)."""
import numpy as np
import pytest
import torch

import sections_reference as sr

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
HOP = 1024
TINY = 2.0 ** -30


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


def signals(R, H, seed):
    """mix, est float32 [R, H * 1024]: Gaussian mixture of sigma 0.1 with |w| >= 2^-30, est = g w with g in [0.2, 0.8] per sample."""
    rng = np.random.RandomState(seed)
    w = (0.1 * rng.randn(R, H * HOP)).astype(np.float32)
    w = np.where(np.abs(w) < TINY, np.float32(TINY), w).astype(np.float32)
    e = (w * rng.uniform(0.2, 0.8, w.shape).astype(np.float32)).astype(np.float32)
    return w, e


def place(a, stride, offset, hops):
    """The rows of `a` in a flat device buffer, `stride` floats apart from `offset` floats in; 5.0 everywhere else and behind hops[r] * 1024
    samples of row r.  Returns the [R, H * 1024] view."""
    R, n = a.shape
    flat = torch.full((offset + R * stride + 8,), 5.0, device="cuda")
    view = flat[offset:offset + R * stride].view(R, stride)[:, :n]
    for r in range(R):
        view[r, :hops[r] * HOP] = torch.from_numpy(a[r, :hops[r] * HOP].copy())
    assert view.data_ptr() == flat.data_ptr() + 4 * offset and (R == 1 or view.stride(0) == stride)
    return view


def run(model, w, e, hops, stride_w, stride_e, offset, pass_hops=True):
    from speechseparation_amd import mining
    R, n = w.shape
    H = n // HOP
    mix, est = place(w, stride_w, offset, hops), place(e, stride_e, offset, hops)
    out = torch.full((R, H, 2), SENTINEL, device="cuda", dtype=torch.float64)
    res = mining.hop_activity(model, mix, est, hops=hops if pass_hops else None, out=out)
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return out.cpu().numpy(), mix, est


@pytest.fixture(scope="module")
def ragged(model):
    """Three rows of 1, 2 and 5 hops in a rectangle of 5, on both load paths and with unequal strides; the reference is computed once."""
    hops, H = [1, 2, 5], 5
    w, e = signals(3, H, seed=3)
    want = sr.activity(w, e, hops=hops)
    scalar, mix_s, est_s = run(model, w, e, hops, H * HOP + 3, H * HOP + 3, 1)
    vector, mix_v, est_v = run(model, w, e, hops, H * HOP + 4, H * HOP + 4, 0)
    mixed, _, _ = run(model, w, e, hops, H * HOP + 8, H * HOP + 256, 4)
    assert mix_s.data_ptr() % 16 == 4 and mix_s.stride(0) % 4 == 3 and mix_v.data_ptr() % 16 == 0 and mix_v.stride(0) % 4 == 0
    return dict(hops=hops, w=w, e=e, want=want, scalar=scalar, vector=vector, mixed=mixed)


def test_one_hop_of_one_row(model):
    w, e = signals(1, 1, seed=1)
    got, _, _ = run(model, w, e, [1], HOP, HOP, 0)
    sr.compare_activity(got, sr.activity(w, e), "R = 1, Hmax = 1")
    # by hand: the first figure is the mean of (e / (w - e))^2 terms, the second the mean square of the mixture
    assert abs(got[0, 0, 1] - np.mean(w.astype(np.float64) ** 2)) < 1e-7 * got[0, 0, 1]


@pytest.mark.parametrize("path", ["scalar", "vector", "mixed"])
def test_ragged_rows_against_the_reference(ragged, path):
    got = ragged[path]
    assert not (got == SENTINEL).any(), "every slot is written"
    sr.compare_activity(got, ragged["want"], "hops (1, 2, 5) of 5, %s loads" % path)
    for r, h in enumerate(ragged["hops"]):
        assert (got[r, h:] == 0.0).all() and (got[r, :h] > 0.0).all()


def test_the_two_load_paths_agree_bit_for_bit(ragged):
    assert np.array_equal(ragged["scalar"], ragged["vector"]) and np.array_equal(ragged["mixed"], ragged["vector"])


def test_what_lies_behind_a_row_is_not_read(model, ragged):
    """The 5.0s behind hops[r] * 1024 samples (place) reached nothing: the same rows over NaNs give the same bits."""
    from speechseparation_amd import mining
    hops, w, e = ragged["hops"], ragged["w"], ragged["e"]
    mix, est = place(w, 5 * HOP + 4, 0, hops), place(e, 5 * HOP + 4, 0, hops)
    for r, h in enumerate(hops):
        mix[r, h * HOP:] = float("nan")
        est[r, h * HOP:] = float("nan")
    got = mining.hop_activity(model, mix, est, hops=hops).cpu().numpy()
    assert np.array_equal(got, ragged["vector"])


def test_no_hop_table_and_a_hop_count_of_zero(model):
    H = 3
    w, e = signals(2, H, seed=5)
    full, _, _ = run(model, w, e, [H, H], H * HOP, H * HOP, 0, pass_hops=False)
    sr.compare_activity(full, sr.activity(w, e), "hops_host = NULL")
    some, _, _ = run(model, w, e, [0, H], H * HOP + 3, H * HOP, 1)
    assert (some[0] == 0.0).all() and np.array_equal(some[1], full[1])
    sr.compare_activity(some, sr.activity(w, e, hops=[0, H]), "hops (0, 3)")
    none, _, _ = run(model, w, e, [0, 0], H * HOP, H * HOP, 0)
    assert (none == 0.0).all()


def test_special_hops_in_one_row(model):
    """est == mix (ratio +inf), est == 0 (ratio exactly 0), both zero (NaN, level 0), one single b == 0 sample among 1023 ordinary ones
    (+inf), an ordinary hop - all in one row."""
    H = 5
    w, e = signals(1, H, seed=7)
    e[0, 0:HOP] = w[0, 0:HOP]
    e[0, HOP:2 * HOP] = 0.0
    w[0, 2 * HOP:3 * HOP] = 0.0
    e[0, 2 * HOP:3 * HOP] = 0.0
    e[0, 3 * HOP + 517] = w[0, 3 * HOP + 517]
    want = sr.activity(w, e)
    assert np.isposinf(want[0, 0, 0]) and want[0, 1, 0] == 0.0 and np.isnan(want[0, 2, 0]) and want[0, 2, 1] == 0.0
    assert np.isposinf(want[0, 3, 0]) and np.isfinite(want[0, 4]).all() and (want[0, [0, 1, 3, 4], 1] > 0).all()
    got, _, _ = run(model, w, e, [H], H * HOP, H * HOP, 0)
    sr.compare_activity(got, want, "special hops")
    assert np.isposinf(got[0, 0, 0]) and got[0, 1, 0] == 0.0 and np.isnan(got[0, 2, 0]) and got[0, 2, 1] == 0.0 and np.isposinf(got[0, 3, 0])


def test_a_second_call_allocates_nothing(model, ragged):
    from speechseparation_amd import _native, mining
    hops, w, e = ragged["hops"], ragged["w"], ragged["e"]
    mix, est = place(w, 5 * HOP + 3, 1, hops), place(e, 5 * HOP + 3, 1, hops)
    out = torch.empty((3, 5, 2), device="cuda", dtype=torch.float64)
    mining.hop_activity(model, mix, est, hops=hops, out=out)
    before = _native.lib.bsrnn_debug_counter(0)
    mining.hop_activity(model, mix, est, hops=hops, out=out)
    mining.hop_activity(model, mix, est, out=out)
    assert _native.lib.bsrnn_debug_counter(0) == before
    torch.cuda.synchronize()


def test_a_row_in_the_batch_equals_the_row_alone(model, ragged):
    hops, w, e = ragged["hops"], ragged["w"], ragged["e"]
    for r, h in enumerate(hops):
        alone, _, _ = run(model, w[r:r + 1, :h * HOP], e[r:r + 1, :h * HOP], [h], h * HOP, h * HOP, 0)
        assert np.array_equal(alone[0], ragged["vector"][r, :h])


def test_python_layer_refuses_bad_arguments(model):
    from speechseparation_amd import _native, mining
    mix, est = torch.zeros((2, 2 * HOP), device="cuda"), torch.zeros((2, 2 * HOP), device="cuda")
    with pytest.raises(ValueError):
        mining.hop_activity(model, mix, est[:1])
    with pytest.raises(ValueError):
        mining.hop_activity(model, mix, est, hops=[1, 3])
    with pytest.raises(ValueError):
        mining.hop_activity(model, mix[:, :100], est)
    with pytest.raises(ValueError):
        mining.hop_activity(model, mix.double(), est)
    with pytest.raises(_native.NativeError):
        mining.hop_activity(model, mix.cpu(), est)
    with pytest.raises(ValueError):
        mining.hop_activity(model, mix, est, out=torch.empty((2, 2, 2), device="cuda"))
