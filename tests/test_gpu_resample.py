"""GPU: sample-rate conversion on the device (BSRNN.resample -> bsrnn_resample, bsrnn.Resampler -> bsrnn_resampler_*,
BSRNN.separate_at_rate, infer.py --model-rate, infer-streaming.py --device-resample).

The reference is scipy.signal.resample_poly of the float64 input - the definition (csrc/resample_host.h).  The bound per output sample
is derived, not tuned:

    |y - ref| <= (L + 2) * 2^-24 * resample_poly(|x|, up, down, window = |h| / up) + L * 2^-149

with L the taps per phase: the fp32 dot-product bound of any summation order over L terms, plus one rounding of each tap (scipy
multiplies an array window by `up` itself, so the second factor is sum |x| |h| of that sample).  A plain fp32 evaluation stays below
0.2 of it; a wrong tap or index does not.  The only comparisons of the library with itself are the equalities the interface promises
(streaming == one-shot, separate_at_rate == its three calls chained, a view == its contiguous copy).

DEPENDENCY of the impulse row: an impulse meets one tap per output, and at the multiples of max(up, down) firwin's tap is the about
1e-17 that sin() leaves of a rounded argument, where the bound is about 1e-23.  The row therefore passes only while the header's
design reproduces those residues, i.e. while the C library's sin() and numpy's agree there to a few ulp.  tests/test_resample_host.py
(test_taps_against_firwin) checks exactly that without a GPU and reports those taps apart: if it and this row fail together after a
change of scipy, numpy or libm, look there first."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import signal

from conftest import REPO

pytestmark = pytest.mark.gpu
PAIRS = [(48000, 44100), (44100, 48000), (16000, 44100), (192000, 44100), (22050, 44100), (44100, 22050), (44100, 44100)]
SIZES = [1, 5, 1500, 20000]
TOL = 1e-4                      # block against step, tests/test_gpu_stream_block.py
TOL_VS_ONE_SHOT = 3e-5          # segmented against one-shot, tests/test_gpu_separate_long.py
EARG = 1


def reduced(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    half = 10 * max(up, down)
    return up, down, half, half // up + (half + up - 1) // up + 1


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


_ROWS = {}


def rows(n):
    """The three test rows of n samples, float32: 0.1 * randn, a full-scale step, a unit impulse at the last sample."""
    if n not in _ROWS:
        x = np.zeros((3, n), np.float32)
        x[0] = 0.1 * np.random.default_rng(100 + n).standard_normal(n)
        x[1, n // 2:] = 1.0
        x[2, -1] = 1.0
        x.setflags(write=False)
        _ROWS[n] = x
    return _ROWS[n]


_REFS = {}


def reference(pair, n):
    """(resample_poly of the float64 rows, the bound per sample), computed once per case."""
    if (pair, n) not in _REFS:
        up, down, half, L = reduced(*pair)
        x = rows(n).astype(np.float64)
        if up == down:          # resample_poly returns the input (and its firwin refuses a cutoff at Nyquist): sum |x| |h| is |x|
            ref, mag = x.copy(), np.abs(x)
        else:
            h = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
            ref = signal.resample_poly(x, up, down, axis=1)
            mag = signal.resample_poly(np.abs(x), up, down, axis=1, window=np.abs(h) / up)
        _REFS[(pair, n)] = (ref, (L + 2) * 2.0 ** -24 * mag + L * 2.0 ** -149)
    return _REFS[(pair, n)]


def run_case(model, pair, n, pad):
    """Rows `n + pad` floats apart with NaN behind the samples; the result goes into rows 5 floats longer than it, prefilled."""
    ref, bound = reference(pair, n)
    n_out = ref.shape[1]
    buf = torch.full((3, n + pad), float("nan"), device="cuda")
    buf[:, :n] = torch.from_numpy(np.array(rows(n))).cuda()
    dst = torch.full((3, n_out + 5), 7.5, device="cuda")
    out = model.resample(buf[:, :n], pair[0], pair[1], out=dst[:, :n_out])
    assert out.data_ptr() == dst.data_ptr() and tuple(out.shape) == (3, n_out)
    got = dst.cpu().numpy()
    assert np.all(got[:, n_out:] == 7.5), "wrote behind n_out"
    y = got[:, :n_out].astype(np.float64)
    assert np.isfinite(y).all(), "something behind n_in reached the output"
    ratio = np.abs(y - ref) / bound
    print("%s n = %d stride n + %d: max |y - ref| / bound = %.3f, per row %s" % (pair, n, pad, ratio.max(), np.round(ratio.max(1), 3)))
    assert (np.abs(y - ref) <= bound).all()
    assert tuple(model.resample(buf[:, :n], pair[0], pair[1]).shape) == (3, n_out)


@pytest.mark.parametrize("pair", PAIRS)
def test_parity_rows_off_alignment(model, pair):
    """in_stride = n_in + 3: odd rows start off 16-byte alignment, so the span is staged by scalar loads.  n_in = 1 and 5 lie wholly inside
    the filter's edge, 1500 is one tile (two at 16 k -> 44.1 k), 20000 several tiles with a ragged last one."""
    for n in SIZES:
        run_case(model, pair, n, 3)


@pytest.mark.parametrize("pair", PAIRS)
def test_parity_rows_aligned(model, pair):
    """in_stride = n_in + 4 with n_in a multiple of 4: every row starts aligned, the span is staged by 16-byte loads."""
    for n in (1500, 20000):
        run_case(model, pair, n, 4)


def test_views_whose_row_stride_is_not_a_row(model):
    """Views whose stride(0) is below the row length - an expanded mono row (stride 0), overlapping rows of an unfold - are copied, not
    handed on with a made-up stride; views that do describe rows (every other row, a column range) are handed on as they are.  Each
    equals the conversion of its contiguous copy, the expanded one also meets the bound against scipy."""
    from speechseparation_amd.bsrnn import Resampler
    pair, n = (48000, 44100), 1500
    ref, bound = reference(pair, n)
    n_out = ref.shape[1]
    mono = torch.from_numpy(np.array(rows(n)[:1])).cuda()
    # one row shown twice: there is no second row n floats further on
    stereo = mono.expand(2, -1)
    assert stereo.stride() == (0, 1)
    y = model.resample(stereo, *pair).cpu().numpy().astype(np.float64)
    assert y.shape == (2, n_out) and (np.abs(y - ref[0]) <= bound[0]).all()
    assert np.array_equal(y[0], y[1])
    rs = Resampler(model, 2, *pair)
    z = torch.cat([rs.process(stereo), rs.flush()], 1).cpu().numpy()
    assert np.array_equal(z, y.astype(np.float32))
    # rows 7 samples apart over one another
    flat = torch.from_numpy(0.1 * np.random.default_rng(5).standard_normal(n + 14).astype(np.float32)).cuda()
    over = flat.unfold(0, n, 7)
    assert tuple(over.shape) == (3, n) and over.stride() == (7, 1)
    assert torch.equal(model.resample(over, *pair), model.resample(over.contiguous(), *pair))
    # every other row of a padded buffer; strided samples
    buf = torch.full((6, n + 3), float("nan"), device="cuda")
    buf[:, :n] = torch.from_numpy(0.1 * np.random.default_rng(6).standard_normal((6, n)).astype(np.float32)).cuda()
    assert torch.equal(model.resample(buf[::2, :n], *pair), model.resample(buf[::2, :n].contiguous(), *pair))
    assert torch.equal(model.resample(buf[:3, 0:n:2], *pair), model.resample(buf[:3, 0:n:2].contiguous(), *pair))
    # a column range whose last row ends where the output begins: the padding "behind" the last row is the output's memory, not the input's
    pad = 8
    store = torch.full((3 * (n + pad) + 3 * n_out,), float("nan"), device="cuda")
    src = store[:3 * (n + pad)].view(3, n + pad)[:, pad:]
    dst = store[3 * (n + pad):].view(3, n_out)
    src.copy_(torch.from_numpy(np.array(rows(n))).cuda())
    assert src.data_ptr() + 4 * 3 * (n + pad) > dst.data_ptr() >= src.data_ptr() + 4 * (2 * (n + pad) + n)
    got = model.resample(src, *pair, out=dst).cpu().numpy().astype(np.float64)
    assert (np.abs(got - ref) <= bound).all()
    # an output whose rows lie over one another is refused before anything runs
    with pytest.raises(ValueError, match="do not overlap"):
        model.resample(src, *pair, out=torch.empty((1, n_out), device="cuda").expand(3, -1))


@pytest.mark.parametrize("pair", [(48000, 44100), (16000, 44100), (192000, 44100)])
def test_streaming_equals_one_shot(model, pair):
    from speechseparation_amd import _native
    from speechseparation_amd.bsrnn import Resampler
    n = 6000
    x = torch.from_numpy(0.1 * np.random.default_rng(7).standard_normal((2, n)).astype(np.float32)).cuda()
    whole = model.resample(x, *pair).cpu().numpy()
    rs = Resampler(model, 2, *pair)
    torch.cuda.synchronize()
    allocs = _native.lib.bsrnn_debug_counter(0)
    blocks = [1, 7, 1024, 0, 333, 2500]
    blocks.append(n - sum(blocks))

    def one_pass():
        outs, pos = [], 0
        for b in blocks:
            want = rs.ready(b)
            y = rs.process(x[:, pos:pos + b])          # a view: rows n floats apart, starting wherever the block starts
            assert tuple(y.shape) == (2, want)
            outs.append(y)
            pos += b
        assert rs.ready(0) == 0
        outs.append(rs.flush())
        return torch.cat(outs, 1).cpu().numpy()
    first = one_pass()
    assert first.shape == whole.shape and np.array_equal(first, whole)
    # a stream broken off, then the same clip again after reset(); a third pass follows the flush without one
    rs.process(x[:, :777])
    rs.reset()
    assert np.array_equal(one_pass(), whole)
    assert np.array_equal(one_pass(), whole)
    assert _native.lib.bsrnn_debug_counter(0) == allocs, "process / flush / reset allocated"


def test_separate_at_rate_is_the_three_calls(model):
    n = 3600                                            # 48 kHz; 3308 samples at 44.1 kHz: four frames, three hops
    x = torch.from_numpy(0.1 * np.random.default_rng(11).standard_normal((2, n)).astype(np.float32)).cuda()
    got = model.separate_at_rate(x, 48000)
    a = model.resample(x, 48000, 44100)
    assert a.shape[1] == 3308
    b = model.separate(a)
    c = model.resample(b, 44100, 48000)
    assert b.shape[1] == 3072 and c.shape[1] == 3344 and tuple(got.shape) == (2, 3344) and got.shape[1] <= n
    assert torch.equal(got, c[:, :n])
    # at the model's rate the call IS separate
    w = torch.from_numpy(0.1 * np.random.default_rng(12).standard_normal((2, 3 * 1024 + 100)).astype(np.float32)).cuda()
    assert torch.equal(model.separate_at_rate(w, 44100), model.separate(w))
    # never longer than the input: 3343 samples are 3072 at the model's rate, three whole hops, which come back as 3344
    short = x[:, :3343].contiguous()
    assert model.resample(short, 48000, 44100).shape[1] == 3072
    y = model.separate_at_rate(short, 48000)
    assert tuple(y.shape) == (2, 3343)
    # in segments: the one-shot result at the tolerance of segmented against one-shot
    seg = model.separate_at_rate(x, 48000, segment_frames=2)
    err = float((seg - got).abs().max())
    print("separate_at_rate segment_frames = 2 against one shot: %.3e" % err)
    assert tuple(seg.shape) == tuple(got.shape) and err < TOL_VS_ONE_SHOT


def _write_wav(path, wave, sr):
    from speechseparation_amd import audio
    audio.save_wav(path, torch.from_numpy(wave), sr)


def test_infer_cli_model_rate(tmp_path, model):
    from speechseparation_amd import audio, weights
    n = 48000 // 8 + 33
    wave = weights.synth_waveform(2, n, seed=21)
    src, dst = str(tmp_path / "in48.wav"), str(tmp_path / "out.wav")
    _write_wav(src, wave, 48000)
    out = subprocess.run([sys.executable, os.path.join(REPO, "infer.py"), "--input", src, "--output", dst, "--synthetic-weights", "0",
                          "--outdir", str(tmp_path), "--model-rate", "44100"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0 and "Separation dB" in out.stdout, out.stderr
    got, sr = audio.load_wav(dst)
    n44 = -(-n * 147 // 160)
    want = min(n, -(-(n44 // 1024 * 1024) * 160 // 147))
    assert sr == 48000 and tuple(got.shape) == (2, want)
    assert torch.equal(got, model.separate_at_rate(torch.from_numpy(wave).cuda(), 48000).cpu())


def test_infer_streaming_cli_device_resample(tmp_path):
    from speechseparation_amd import audio, weights
    wave = weights.synth_waveform(2, 48000 // 8 + 33, seed=12)           # the clip of test_infer_streaming_cli_resamples_to_44k1
    src = str(tmp_path / "in48.wav")
    _write_wav(src, wave, 48000)
    got = []
    for extra in ([], ["--device-resample"]):
        dst = str(tmp_path / ("out%d.wav" % len(got)))
        out = subprocess.run([sys.executable, os.path.join(REPO, "infer-streaming.py"), "--input", src, "--output", dst, "--name", "t",
                              "--synthetic-weights", "0", "--export", ""] + extra, capture_output=True, text=True, timeout=300, cwd=REPO)
        assert out.returncode == 0, out.stderr
        y, sr = audio.load_wav(dst)
        assert sr == 44100
        got.append(y)
    assert got[0].shape == got[1].shape and got[0].shape[1] >= 5 * 1024
    err = float((got[0] - got[1]).abs().max())
    print("infer-streaming.py host against device resampling: %.3e" % err)
    assert err < TOL


def test_refusals(model):
    from speechseparation_amd import _native
    from speechseparation_amd.bsrnn import Resampler
    lib = _native.lib
    x = torch.zeros((2, 1000), device="cuda")
    ctx = model._context(x.device)
    torch.cuda.synchronize()
    sentinel = torch.full((2, 1000), 3.0, device="cuda")
    vp = ctypes.c_void_p

    def err():
        return lib.bsrnn_last_error().decode()
    # the output over the input: in place, and only its last sample
    assert lib.bsrnn_resample(ctx, vp(x.data_ptr()), 1000, vp(x.data_ptr()), 1000, 2, 1000, 48000, 44100, None) == EARG
    assert "overlap" in err()
    assert lib.bsrnn_resample(ctx, vp(x.data_ptr()), 1000, vp(x.data_ptr() + 4 * 1999), 1000, 2, 1000, 48000, 44100, None) == EARG
    assert "overlap" in err()
    # a ratio that does not reduce to 1024 or less
    assert lib.bsrnn_resample(ctx, vp(x.data_ptr()), 1000, vp(sentinel.data_ptr()), 1000, 2, 100, 44100, 48001, None) == EARG
    assert "48001 / 44100" in err() and "1024" in err()
    with pytest.raises(ValueError):
        model.resample(x, 44100, 48001)
    with pytest.raises(ValueError):
        Resampler(model, 2, 44100, 48001)
    h = vp()
    assert lib.bsrnn_resampler_create(ctx, 2, 44100, 48001, ctypes.byref(h)) == EARG and not h.value
    assert lib.bsrnn_resampler_create(ctx, 0, 48000, 44100, ctypes.byref(h)) == EARG and not h.value
    assert "C = 0" in err()
    # a block whose rows are not the resampler's; its output over its input; an output row too short for the count
    rs = Resampler(model, 2, 48000, 44100)
    with pytest.raises(ValueError, match=r"C = 2"):
        rs.process(torch.zeros((3, 100), device="cuda"))
    n = ctypes.c_int64(-1)
    assert lib.bsrnn_resampler_process(rs._h, vp(x.data_ptr()), 1000, 1000, vp(x.data_ptr() + 4 * 500), 1000, ctypes.byref(n), None) == EARG
    assert "overlap" in err() and n.value == -1
    assert lib.bsrnn_resampler_process(rs._h, vp(x.data_ptr()), 1000, 1000, vp(sentinel.data_ptr()), 10, ctypes.byref(n), None) == EARG
    assert "out_stride" in err() and n.value == -1
    assert lib.bsrnn_resampler_process(rs._h, vp(x.data_ptr()), 1000, -1, vp(sentinel.data_ptr()), 1000, ctypes.byref(n), None) == EARG
    # nothing was launched and nothing taken: the refused blocks left no trace
    torch.cuda.synchronize()
    assert rs.ready(0) == 0 and rs.flush().shape[1] == 0
    assert bool((sentinel == 3.0).all()) and not bool(x.any())
