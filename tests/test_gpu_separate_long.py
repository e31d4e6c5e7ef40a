"""GPU: long-form separation (BSRNN.separate_long -> bsrnn_separate_long / bsrnn_separate_long_host): bsrnn_separate's result from a
workspace of one segment.  Expected values are the numpy oracle's one-shot sandwich (oracle/bsrnn_numpy.separate) on seeded inputs;
the only comparisons of the library with itself are the bit-equalities the interface promises (one segment == separate, host path ==
device path, run == re-run).

Bounds: 1e-4 max-abs against the oracle is the project's waveform contract (tests/test_gpu_parity.py, TOL).  3e-5 against the one-shot
`separate` is the bound tests/test_gpu_edges.py::test_long_sequence_causality holds chunked-with-carry spectra to against the offline
forward; the iSTFT cannot enlarge a max-abs spectral error (a sample is a sum of 2050 terms over 2048, times window weights that sum
to one over the two frames that cover it)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, golden

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_VS_ONE_SHOT = 3e-5
R0, N0, T0 = 2, 9 * 1024 + 77, 10         # the default case: T = 10 frames
EARG = 1


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def make_model(sd, v=None):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN(v).eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}, strict=True)
    return m.to("cuda")


@pytest.fixture(scope="module")
def model(sd_default):
    return make_model(sd_default)


_CASES = {}


def case(sd, rows, n):
    """(waveform, oracle result) of a seeded clip, computed once per shape and left unchanged."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    if (rows, n) not in _CASES:
        wave = weights.synth_waveform(rows, n, seed=300 + rows + n % 1000)
        ref = onp.separate(sd, wave)
        wave.setflags(write=False)
        ref.setflags(write=False)
        _CASES[(rows, n)] = (wave, ref)
    return _CASES[(rows, n)]


def dev(wave):
    return torch.from_numpy(np.array(wave)).cuda()


@pytest.mark.parametrize("seg", [1, 2, 3, 7, T0 - 1])
def test_parity_at_every_cut(model, sd_default, seg):
    wave, ref = case(sd_default, R0, N0)
    out = model.separate_long(dev(wave), seg).cpu().numpy()
    one = model.separate(dev(wave)).cpu().numpy()
    e_ref, e_one = maxabs(out, ref), maxabs(out, one)
    print("seg_frames %d: max|long - oracle| %.3e, max|long - separate| %.3e" % (seg, e_ref, e_one))
    assert out.shape == ref.shape == (R0, (T0 - 1) * 1024)
    assert e_ref < TOL
    assert e_one < TOL_VS_ONE_SHOT


@pytest.mark.parametrize("seg", [1, 3])
@pytest.mark.parametrize("rows,n", [(2, 8 * 1024), (2, 8 * 1024 + 1), (2, 8 * 1024 + 1023), (2, 1025), (3, 4 * 1024 + 77)])
def test_clip_ends(model, sd_default, rows, n, seg):
    """The clip's last frame reflects at n - 1 - for n a multiple of 1024 to one sample in front of the frame's own first -, the
    minimum length has two frames, and an odd row count fills no tile."""
    wave, ref = case(sd_default, rows, n)
    out = model.separate_long(dev(wave), seg).cpu().numpy()
    e = maxabs(out, ref)
    print("R %d n %d seg_frames %d: max|long - oracle| %.3e" % (rows, n, seg, e))
    assert out.shape == ref.shape == (rows, (n // 1024) * 1024)
    assert e < TOL


def test_one_segment_is_separate_and_runs_repeat(model, sd_default):
    wave, _ = case(sd_default, R0, N0)
    w = dev(wave)
    one = model.separate(w)
    for seg in (T0, T0 + 4):
        assert torch.equal(model.separate_long(w, seg), one), seg
    a, b = model.separate_long(w, 3), model.separate_long(w, 3)
    assert torch.equal(a, b)
    assert np.array_equal(w.cpu().numpy(), wave)                    # the input is not modified


@pytest.mark.parametrize("seg", [1, 3, 7])
def test_host_path_equals_device_path(model, sd_default, seg):
    wave, ref = case(sd_default, R0, N0)
    host_in = torch.from_numpy(np.array(wave))
    host = model.separate_long(host_in, seg)
    assert not host.is_cuda and host.dtype == torch.float32
    assert torch.equal(host, model.separate_long(dev(wave), seg).cpu())
    e = maxabs(host.numpy(), ref)
    print("host path, seg_frames %d: max|long - oracle| %.3e" % (seg, e))
    assert e < TOL
    assert np.array_equal(host_in.numpy(), wave)


def test_host_path_one_segment_and_out_argument(model, sd_default):
    wave, _ = case(sd_default, R0, N0)
    one = model.separate(dev(wave)).cpu()
    out = torch.empty_like(one)
    got = model.separate_long(torch.from_numpy(np.array(wave)), T0 + 4, out=out)
    assert got is out and torch.equal(out, one)
    with pytest.raises(ValueError):
        model.separate_long(torch.from_numpy(np.array(wave)), 3, out=torch.empty((R0, 5)))
    with pytest.raises(ValueError):
        model.separate_long(dev(wave), 3, out=torch.empty_like(one))             # out on another device than the waveform


def test_bounded_memory(sd_default):
    """The workspace and the first-use allocations are those of one segment: a clip three times as long changes neither, on either
    path; the one-shot call of that clip needs R * T rows (which shows that the getter measures what it claims)."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import _native, weights
    m = make_model(sd_default)                                        # a fresh context
    wave, ref = case(sd_default, R0, N0)
    assert m.workspace_rows() == 0
    assert maxabs(m.separate_long(dev(wave), 3).cpu().numpy(), ref) < TOL
    assert 0 < m.workspace_rows() <= R0 * 3
    m.separate_long(torch.from_numpy(np.array(wave)), 3)              # (the host path's staging: first use)
    rows, allocs = m.workspace_rows(), _native.lib.bsrnn_debug_counter(0)
    n3 = 3 * N0
    T3 = 1 + n3 // 1024
    long_wave = weights.synth_waveform(R0, n3, seed=41)
    long_ref = onp.separate(sd_default, long_wave)
    out_dev = m.separate_long(torch.from_numpy(long_wave).cuda(), 3)
    assert (m.workspace_rows(), _native.lib.bsrnn_debug_counter(0)) == (rows, allocs)
    out_host = m.separate_long(torch.from_numpy(long_wave), 3)
    assert (m.workspace_rows(), _native.lib.bsrnn_debug_counter(0)) == (rows, allocs)
    assert maxabs(out_dev.cpu().numpy(), long_ref) < TOL and torch.equal(out_host, out_dev.cpu())
    m.separate(torch.from_numpy(long_wave).cuda())
    assert m.workspace_rows() >= R0 * T3


def test_range_policy_per_segment(model, sd_default):
    """Samples 3*1024 .. 5*1024 - 1 reach frames 3, 4 and 5 only: with three frames per segment exactly the second segment.  Scaled by
    3e5 they drive its spectrum to |x| ~ 1e7, beyond the fp16x2 operand range; under the default policy that segment is run again on
    the exact-fp32 kernels from its untouched state and carry set, and the call returns rc 0 with the reference's numbers.  The bound
    is the one tests/test_gpu_edges.py::test_synchronous_entry_points_rerun_out_of_range_calls_in_fp32 holds `separate` (through
    evaluate) to: 2e-6 of the reference's largest value, against the float64 oracle."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import _native
    if _native.compute_mode()["gemm"] != "fp16x2":
        pytest.skip("range guard belongs to the fp16x2 mode")
    wave = np.array(case(sd_default, R0, N0)[0], np.float64)
    wave[:, 3 * 1024:5 * 1024] *= 3e5
    big = wave.astype(np.float32)
    ref = onp.separate(sd_default, big, dtype=np.float64)
    for name, x in (("device", torch.from_numpy(big).cuda()), ("host", torch.from_numpy(big))):
        out = model.separate_long(x, 3).cpu().numpy()                # (a non-zero rc raises NativeError)
        rel = maxabs(out, ref) / np.abs(ref).max()
        print("%s path: |ref|max %.3g relative error %.2e" % (name, np.abs(ref).max(), rel))
        assert rel < 2e-6, (name, rel)
    # nothing is left pending: the next call on the context succeeds
    model.separate(dev(case(sd_default, R0, N0)[0]))


def test_no_carry_leaks_between_clips(model, sd_default):
    (w1, r1), (w2, r2) = case(sd_default, R0, N0), case(sd_default, 2, 8 * 1024 + 1)
    for path in (dev, lambda w: torch.from_numpy(np.array(w))):
        assert maxabs(model.separate_long(path(w1), 3).cpu().numpy(), r1) < TOL
        assert maxabs(model.separate_long(path(w2), 3).cpu().numpy(), r2) < TOL
        assert maxabs(model.separate_long(path(w1), 3).cpu().numpy(), r1) < TOL


def test_argument_errors(model, sd_default):
    from speechseparation_amd import _native
    lib = _native.lib
    wave, _ = case(sd_default, R0, N0)
    w = dev(wave)
    out = torch.empty((R0, (T0 - 1) * 1024), device="cuda")
    ctx = model._context(torch.device("cuda", torch.cuda.current_device()))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.bsrnn_separate_long(ctx, p(w), p(out), R0, N0, 0, None) == EARG
    assert b"seg_frames" in lib.bsrnn_last_error()
    assert lib.bsrnn_separate_long(ctx, p(w), p(w), R0, N0, 3, None) == EARG            # out overlapping wave
    assert b"overlap" in lib.bsrnn_last_error()
    assert lib.bsrnn_separate_long(ctx, p(w), p(out), R0, 1024, 3, None) == EARG        # n = 1024: no reflect padding
    hw, ho = np.array(wave), np.empty((R0, (T0 - 1) * 1024), np.float32)
    q = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.bsrnn_separate_long_host(ctx, q(hw), q(ho), R0, N0, 0) == EARG
    assert lib.bsrnn_separate_long_host(ctx, q(hw), q(hw), R0, N0, 3) == EARG
    assert lib.bsrnn_separate_long_host(ctx, q(hw), q(ho), R0, 1024, 3) == EARG
    # under the deferred policy too: the overlap is unsafe whatever the policy
    model.set_range_policy("deferred")
    try:
        assert lib.bsrnn_separate_long(ctx, p(w), p(w), R0, N0, 3, None) == EARG
    finally:
        model.set_range_policy("exact")
    with pytest.raises(_native.NativeError):
        model.separate_long(w, 0)                                                       # the C layer's error, through the wrapper
    with pytest.raises(ValueError):
        model.separate_long(w[0], 3)                                                    # a shape error
    torch.cuda.synchronize()
    assert np.array_equal(w.cpu().numpy(), wave)


def test_deferred_policy_matches(model, sd_default):
    """Under the deferred policy no segment waits; an in-range clip gives the same samples."""
    wave, ref = case(sd_default, R0, N0)
    exact = model.separate_long(dev(wave), 3)
    model.set_range_policy("deferred")
    try:
        a = model.separate_long(dev(wave), 3)
        b = model.separate_long(torch.from_numpy(np.array(wave)), 3)
        model.sync()
    finally:
        model.set_range_policy("exact")
    assert torch.equal(a, exact) and torch.equal(b, exact.cpu())


def test_bands41():
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    v = [int(a) for a in golden("bands41_T3")["v"]]
    sd = weights.synth_state_dict(v, seed=3)
    m = make_model(sd, v)
    wave = weights.synth_waveform(2, 5 * 1024 + 33, seed=17)         # T = 6
    ref = onp.separate(sd, wave, v)
    for x in (torch.from_numpy(wave).cuda(), torch.from_numpy(wave)):
        e = maxabs(m.separate_long(x, 2).cpu().numpy(), ref)
        print("41 bands, %s path: max|long - oracle| %.3e" % ("device" if x.is_cuda else "host", e))
        assert e < TOL


def test_infer_cli_segment_frames(tmp_path, model, sd_default):
    """infer.py --segment-frames 3 on a stereo file of T = 10 frames: the written file holds separate_long's samples of the same data."""
    from speechseparation_amd import audio
    wave, ref = case(sd_default, R0, N0)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    audio.save_wav(src, torch.from_numpy(np.array(wave)), 16000)
    out = subprocess.run([sys.executable, os.path.join(REPO, "infer.py"), "--input", src, "--output", dst, "--synthetic-weights", "0",
                          "--outdir", str(tmp_path), "--segment-frames", "3"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr
    assert "Separation dB" in out.stdout
    got, sr = audio.load_wav(dst)
    loaded, _ = audio.load_wav(src)
    assert sr == 16000 and np.array_equal(loaded.numpy(), wave)
    assert torch.equal(got, model.separate_long(loaded, 3))
    assert maxabs(got.numpy(), ref) < TOL
    for tag in ("100", "90", "50", "20", "-100"):
        assert os.path.exists(str(tmp_path / ("mix_%s.wav" % tag)))
