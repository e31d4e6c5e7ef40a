"""GPU: the kernels of csrc/fft.hip alone - offline STFT and iSTFT, the two layout transposes, the iSTFT backward and the
streaming DSP (one hop and blocks) - against the float64 evaluation of the same operation on the CPU, at the sizes where the
kernels change behaviour.  Criterion, references, case table and seeded inputs: tests/test_dsp_reference.py, which also shows
on the CPU that a float32 radix-4 evaluation meets the criterion.  Every tolerance here comes from the float32 evaluation of
the reference, none from the kernels.

Entry points: BSRNN.stft (stft_kernel + layout from frame-major), BSRNN.istft (layout to frame-major + istft_fused_kernel),
train.IstftFunction (the backward's prescale, zero-padded STFT, postscale, layout) and StreamingSeparator (the four streaming
kernels).  The segment kernels are reachable only with the model in between; test_gpu_separate_long.py keeps them."""
import numpy as np
import pytest
import torch

import test_dsp_reference as dsp
from test_dsp_reference import F2, HOP

pytestmark = pytest.mark.gpu


def t2n(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


# ------------------------------------------------------------------------------------------ a. bsrnn_stft
@pytest.mark.parametrize("R,n,signal", dsp.stft_runs())
def test_stft_against_float64(model, R, n, signal):
    wave = dsp.waveform(R, n, signal)
    w = torch.from_numpy(wave).cuda()
    x = model.stft(w)
    T = dsp.frames_of(n)
    assert tuple(x.shape) == (R, F2, T) and x.dtype == torch.float32
    assert torch.equal(w.cpu(), torch.from_numpy(wave))                       # the input is unchanged
    assert not bool(x[:, 1, :].any()) and not bool(x[:, 2049, :].any())       # Im of bins 0 and 1024: exactly zero
    dsp.hold("stft R=%d n=%d T=%d %s" % (R, n, T, signal), t2n(x), dsp.ref_stft(wave, torch.float32), dsp.ref_stft(wave, torch.float64),
             per="frame")


# ------------------------------------------------------------------------------------------ b. bsrnn_istft
@pytest.mark.parametrize("R,T", dsp.istft_shapes())
def test_istft_against_float64(model, R, T):
    y = dsp.spectrum(R, T)
    assert float(np.abs(y[:, 1, :]).min()) > 0 and float(np.abs(y[:, 2049, :]).min()) > 0
    yd = torch.from_numpy(y).cuda()
    w = model.istft(yd)
    assert tuple(w.shape) == (R, (T - 1) * HOP) and w.dtype == torch.float32
    assert torch.equal(yd.cpu(), torch.from_numpy(y))
    dsp.hold("istft R=%d T=%d" % (R, T), t2n(w), dsp.ref_istft(y, torch.float32), dsp.ref_istft(y, torch.float64), per="hop")
    # the imaginary parts of bins 0 and 1024 are ignored, as c2r ignores them: without them, the same bits
    yz = yd.clone()
    yz[:, 1, :] = 0
    yz[:, 2049, :] = 0
    assert torch.equal(model.istft(yz), w)


# ------------------------------------------------------------------------------------------ c. bit relations
def test_a_frame_has_the_same_bits_in_every_launch(model):
    """Every frame's arithmetic is the same whatever launch it sits in: the frames of a clip's head that read no sample past
    the head equal the same frames of the whole clip bit for bit (the head's T selects layout_kernel at 20, layout_wide_kernel
    with 16-byte rows at 40 and with scalar odd rows at 41; the whole clip's T = 139 takes the tiled, whole == false form), and
    so do the hops of a spectrum's head - all (T1 - 1) of them: hop b reads frames b and b + 1 only."""
    T = 139
    wave = dsp.waveform(3, (T - 1) * HOP + 300, seed=31)
    w = torch.from_numpy(wave).cuda()
    x = model.stft(w)
    assert x.shape[2] == T
    for T1 in (20, 40, 41):
        n1 = (T1 - 1) * HOP + 100
        t = (n1 - HOP) // HOP + 1                                             # frames with t * 1024 + 1023 < n1
        assert t == T1 - 1 and (t - 1) * HOP + 1023 < n1 <= t * HOP + 1023
        head = model.stft(w[:, :n1].contiguous())
        assert head.shape[2] == T1
        assert torch.equal(head[:, :, :t], x[:, :, :t]), T1
    y = torch.from_numpy(dsp.spectrum(3, T, seed=32)).cuda()
    full = model.istft(y)
    for T1 in (6, 20, 41):
        head = model.istft(y[:, :, :T1].contiguous())
        assert tuple(head.shape) == (3, (T1 - 1) * HOP)
        assert torch.equal(head, full[:, :(T1 - 1) * HOP]), T1


def test_a_row_has_the_same_bits_alone_and_in_the_large_batch(model):
    """Rows 0, 41 and 79 of the 80-row case run alone (4 frames per workgroup) against the same rows of the batch (whose
    R * ceil(T / 4) workgroups exceed the resident slots, so a workgroup walks more than 4 frames), STFT and iSTFT."""
    R, n = dsp.STFT_CASES[-1]
    assert R == 80
    T = dsp.frames_of(n)
    w = torch.from_numpy(dsp.waveform(R, n)).cuda()
    y = torch.from_numpy(dsp.spectrum(R, T)).cuda()
    x, v = model.stft(w), model.istft(y)
    for r in (0, 41, 79):
        assert torch.equal(model.stft(w[r:r + 1].contiguous()), x[r:r + 1]), r
        assert torch.equal(model.istft(y[r:r + 1].contiguous()), v[r:r + 1]), r


# ------------------------------------------------------------------------------------------ d. bsrnn_istft_backward
@pytest.mark.parametrize("R,T", dsp.BACKWARD_CASES)
def test_istft_backward_against_float64_autograd(R, T):
    from speechseparation_amd import train                  # (its own context, with the default band table)
    y = dsp.spectrum(R, T, seed=3000 + T)
    g = dsp.gaussian((R, (T - 1) * HOP), 3100 + T)
    yg = torch.from_numpy(y).cuda().requires_grad_(True)
    (train.IstftFunction.apply(yg) * torch.from_numpy(g).cuda()).sum().backward()
    assert tuple(yg.grad.shape) == (R, F2, T)
    # the imaginary parts of bins 0 and 1024 get no gradient (irfft ignores them)
    assert not bool(yg.grad[:, 1, :].any()) and not bool(yg.grad[:, 2049, :].any())
    g64 = dsp.ref_istft_grad(y, g, torch.float64)
    assert not g64[:, 1, :].any() and not g64[:, 2049, :].any()
    dsp.hold("istft backward R=%d T=%d" % (R, T), t2n(yg.grad), dsp.ref_istft_grad(y, g, torch.float32), g64)


# ------------------------------------------------------------------------------------------ e. streaming DSP as a pure delay
def _delayed(x):
    """The input delayed by one hop behind a hop of zeros, in float64: what the streaming DSP computes in exact arithmetic."""
    x = np.asarray(x, np.float64)
    return np.concatenate((np.zeros((x.shape[0], HOP)), x[:, :-HOP]), 1)


@pytest.mark.parametrize("C,pattern,host", [
    (2, [1] * 6, False),                    # six step calls on device tensors
    (2, [1] * 6, True),                     # six step calls on host tensors (bsrnn_stream_step_host)
    (1, [17], False),                       # one process call of 17 hops
    (3, [9], False),
    (2, [3, 1, 5, 1, 1, 8], False),         # a 1 is a step, the rest process: the step / block hand-over in both directions
    (3, [5, 2], False),
])
def test_streaming_dsp_is_a_one_hop_delay(model, C, pattern, host):
    """mix = 0.0: both synthesis kernels form 0 * y + 1 * x, the analysed spectrum itself (the model's output is finite), so
    the stream computes irfft(rfft(buf * hann)) overlap-added and divided by the window sum: the input one hop late.  That
    needs no model, and holds the carried analysis buffer, the previous frame, the block kernels' chunk edges and the hand-over
    between step and block at rounding level.  After reset(): zeros, then the first new hop."""
    from speechseparation_amd.bsrnn import StreamingSeparator
    L = sum(pattern)
    x = dsp.gaussian((C, L * HOP), 4000 + 100 * C + 10 * len(pattern) + host)
    z = dsp.gaussian((C, 2 * HOP), 4500 + C)
    st = StreamingSeparator(model, channels=C)
    place = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if host else (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda())

    def feed(sig, hops):
        outs, pos = [], 0
        for h in hops:
            piece = place(sig[:, pos * HOP:(pos + h) * HOP])
            out = st.step(piece, mix=0.0) if h == 1 else st.process(piece, mix=0.0)
            assert tuple(out.shape) == (C, h * HOP) and out.is_cuda == (not host)
            outs.append(t2n(out))
            pos += h
        return np.concatenate(outs, 1)

    got = feed(x, pattern)
    st.reset()
    got = np.concatenate((got, feed(z, [1, 1] if max(pattern) == 1 else [2])), 1)
    assert np.isfinite(got).all()
    ref64 = np.concatenate((_delayed(x), _delayed(z)), 1)
    ref32 = np.concatenate((dsp.ref_delay_loop(x, torch.float32), dsp.ref_delay_loop(z, torch.float32)), 1)
    # (the float64 loop is the shifted input to 1e-15: the reference needs no transform at all)
    assert np.abs(np.concatenate((dsp.ref_delay_loop(x, torch.float64), dsp.ref_delay_loop(z, torch.float64)), 1) - ref64).max() < 1e-13
    dsp.hold("stream C=%d %s %s" % (C, pattern, "host" if host else "device"), got, ref32, ref64)
