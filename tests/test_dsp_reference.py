"""The DSP kernels' criterion, their case inputs and a CPU proof that the criterion is fair (no GPU needed).

csrc/fft.hip is held (tests/test_gpu_dsp.py) to the float64 evaluation of the same operation on the CPU - torch.stft /
torch.istft with the periodic Hann 2048 window, hop 1024, centre and reflect, as oracle/bsrnn_torch_cpu.py calls them - with
the same torch call in float32 as the comparator:

    e_hip <= 3 * e_f32 + 2**-24 * max|ref64|         e_hip = max|hip - ref64|,  e_f32 = max|ref32 - ref64|

The factor 3 is the project's (test_gpu_parity.py::test_precision_is_at_fp32_rounding_level); the floor is half an ulp of the
largest output, the rounding of the result alone (these outputs span 1e-2 .. 1e3, so an absolute floor would not do).  The same
with L2 norms per frame (STFT) and per hop (iSTFT), so that one bad frame cannot hide under another frame's peak.

This file holds what both test files share - the case table, the seeded inputs, the references, the criterion - and restates
the forward kernel's arithmetic in numpy float32 (window, five radix-4 Stockham passes, real split, in the kernel's operation
order, tables rounded from double).  That restatement meets the criterion on every STFT case: a correct radix-4 float32
evaluation can satisfy the bound, and a later tightening of the bound past what the algorithm gives fails here first."""
import numpy as np
import pytest
import torch

HOP, NFFT, NBINS, F2 = 1024, 2048, 1025, 2050
FACTOR = 3.0
HALF_ULP = 2.0 ** -24

# (R, n): T = 1 + n // 1024 and what the size crosses in csrc/fft.hip
STFT_CASES = [
    (1, 1025),                 # T 2: minimum length; tail chunk of 2
    (3, 2047),                 # T 2: end reflection 2 (n - 1) - idx over 1023 samples
    (2, 2048),                 # T 3: n % 1024 == 0
    (1, 4 * 1024 + 1),         # T 5: chunk of 4 plus a one-frame tail (dummy reload)
    (3, 8 * 1024 + 1023),      # T 9: 4 + 4 + 1
    (3, 30 * 1024 + 5),        # T 31: last T on layout_kernel
    (3, 31 * 1024),            # T 32: first T on layout_wide_kernel, all vec4
    (3, 32 * 1024 + 77),       # T 33: odd T: row 1 scalar, rows 0 and 2 vec4, nf = 2 tile scalar
    (2, 33 * 1024 + 1),        # T 34: even T, T % 4 == 2
    (2, 126 * 1024 + 3),       # T 127: odd, whole tile
    (3, 127 * 1024),           # T 128: nt == LT
    (3, 128 * 1024 + 9),       # T 129: whole == false, nt tail of 1
    (80, 124 * 1024 + 500),    # T 125: R * ceil(T / 4) = 2560 workgroups exceed the resident slots: more than 4 frames each
]
SIGNALS = ("gaussian", "constant", "alternating", "tone", "quiet")
SIGNAL_CASE = (3, 8 * 1024 + 1023)          # the size at which every signal of SIGNALS is run; the others run "gaussian"
BACKWARD_CASES = [(1, 2), (3, 5), (2, 9), (3, 33)]


def frames_of(n):
    return 1 + n // HOP


def stft_runs():
    """(R, n, signal) of every STFT run, in a fixed order."""
    runs = [(R, n, "gaussian") for R, n in STFT_CASES]
    return runs + [SIGNAL_CASE + (s,) for s in SIGNALS[1:]]


def istft_shapes():
    """(R, T) of every iSTFT run: the T list and the R of the STFT cases."""
    return [(R, frames_of(n)) for R, n in STFT_CASES]


def gaussian(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def waveform(R, n, signal="gaussian", seed=None):
    """The input of one STFT run, float32 [R, n], from a seed that depends on the case alone."""
    seed = 1000 + 7 * R + n if seed is None else seed
    k = np.arange(n, dtype=np.float64)
    if signal == "gaussian":
        return gaussian((R, n), seed)
    if signal == "constant":
        return np.ones((R, n), np.float32)
    if signal == "alternating":
        return np.tile(np.where(k % 2 == 0, 1.0, -1.0).astype(np.float32), (R, 1))
    if signal == "tone":
        tone = 0.9 * np.sin(2 * np.pi * 440.0 * k / 16000.0)
        return (tone[None, :] + 1e-4 * gaussian((R, n), seed).astype(np.float64)).astype(np.float32)
    if signal == "quiet":
        return gaussian((R, n), seed, 1e-4)
    raise ValueError(signal)


def spectrum(R, T, seed=None):
    """The input of one iSTFT run: gaussian of standard deviation 30 in every column, the imaginary parts of bins 0 and 1024
    included (c2r ignores them) - not the STFT of anything."""
    return gaussian((R, F2, T), 2000 + 11 * R + T if seed is None else seed, 30.0)


# ------------------------------------------------------------------------------------------ references (torch on the CPU)
def interleave(X):
    """complex [R, 1025, T] -> [R, 2050, T], column 2f = re, 2f + 1 = im (infer.py:29-33)."""
    return torch.stack((X.real, X.imag), dim=2).reshape(X.shape[0], F2, X.shape[2])


def deinterleave(y):
    yc = y.reshape(y.shape[0], NBINS, 2, y.shape[2])
    return torch.complex(yc[:, :, 0, :], yc[:, :, 1, :])


def ref_stft(wave, dtype):
    w = torch.from_numpy(np.asarray(wave)).to(dtype)
    X = torch.stft(w, n_fft=NFFT, hop_length=HOP, window=torch.hann_window(NFFT, dtype=dtype), center=True, pad_mode="reflect",
                   return_complex=True)
    return interleave(X).numpy()


def ref_istft(y, dtype):
    Y = deinterleave(torch.from_numpy(np.asarray(y)).to(dtype))
    return torch.istft(Y, n_fft=NFFT, hop_length=HOP, window=torch.hann_window(NFFT, dtype=dtype), center=True).numpy()


def ref_istft_grad(y, g, dtype):
    """d sum(istft(y) * g) / dy by autograd."""
    yt = torch.from_numpy(np.asarray(y)).to(dtype).requires_grad_(True)
    w = torch.istft(deinterleave(yt), n_fft=NFFT, hop_length=HOP, window=torch.hann_window(NFFT, dtype=dtype), center=True)
    (w * torch.from_numpy(np.asarray(g)).to(dtype)).sum().backward()
    return yt.grad.numpy()


def ref_delay_loop(x, dtype):
    """The streaming DSP without a model (infer-streaming.py:116-145 with the spectrum passed through): x [C, L * 1024] ->
    irfft(rfft(buf * hann)) overlap-added with no synthesis window and divided by the window sum, hop after hop."""
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    C = xt.shape[0]
    win = torch.hann_window(NFFT, dtype=dtype)
    buf, prev, outs = torch.zeros((C, NFFT), dtype=dtype), torch.zeros((C, NFFT), dtype=dtype), []
    for l in range(xt.shape[1] // HOP):
        buf = torch.cat((buf[:, HOP:], xt[:, l * HOP:(l + 1) * HOP]), 1)
        s = torch.fft.irfft(torch.fft.rfft(buf * win, dim=1), n=NFFT, dim=1)
        outs.append((s[:, :HOP] + prev[:, HOP:]) / (win[:HOP] + win[HOP:]))
        prev = s
    return torch.cat(outs, 1).numpy()


# ------------------------------------------------------------------------------------------ the criterion
def _units(a, per):
    """[units, samples] view of a result: per 'frame' [R, 2050, T] -> rows (r, t); per 'hop' [R, H * 1024] -> rows (r, h)."""
    if per == "frame":
        return a.transpose(0, 2, 1).reshape(-1, a.shape[1])
    if per == "hop":
        return a.reshape(-1, HOP)
    raise ValueError(per)


def measure(what, got, ref32, ref64, per=None):
    """Print and return the figures of the criterion: e_hip, e_f32, the max-abs bound, and with `per` the worst unit's
    (L2 error - floor) / (L2 error of float32)."""
    got, ref32, ref64 = (np.asarray(a, np.float64) for a in (got, ref32, ref64))
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref32.shape, ref64.shape)
    d, d32 = got - ref64, ref32 - ref64
    m = {"e": float(np.abs(d).max()), "e32": float(np.abs(d32).max()), "peak": float(np.abs(ref64).max())}
    m["bound"] = FACTOR * m["e32"] + HALF_ULP * m["peak"]
    m["ratio"] = m["e"] / m["e32"] if m["e32"] > 0 else float("inf") if m["e"] > 0 else 0.0
    line = "%s: e %.3e  e_f32 %.3e  ratio %.2f  (max|ref| %.3g, bound %.3e)" % (what, m["e"], m["e32"], m["ratio"], m["peak"], m["bound"])
    if per:
        l2 = lambda a: np.sqrt(np.square(_units(a, per)).sum(1))      # noqa: E731
        u, u32, uref = l2(d), l2(d32), l2(ref64)
        slack = FACTOR * u32 + HALF_ULP * uref - u
        w = int(np.argmin(slack))
        m.update(unit=w, unit_e=float(u[w]), unit_bound=float(u[w] + slack[w]), unit_ok=bool(slack[w] >= 0),
                 unit_ratio=float(np.max(u / np.maximum(u32, 1e-300))))
        line += "  per %s: worst L2 ratio %.2f, tightest unit %d: %.3e <= %.3e" % (per, m["unit_ratio"], w, m["unit_e"], m["unit_bound"])
    print(line)
    return m


def hold(what, got, ref32, ref64, per=None):
    """Assert the criterion, in max-abs form and (with `per`) in its L2-per-unit form; returns the figures."""
    m = measure(what, got, ref32, ref64, per)
    assert m["e"] <= m["bound"], (what, m)
    if per:
        assert m["unit_ok"], (what, m)
    return m


# ------------------------------------------------------------------------------------------ the kernel's forward arithmetic
def kernel_tables():
    """tw1024, tw2048 and the window as bsrnn_create builds them: evaluated in double, rounded to float."""
    k = np.arange(1024, dtype=np.float64)
    k2 = np.arange(1025, dtype=np.float64)
    i = np.arange(NFFT, dtype=np.float64)
    f = np.float32
    return {"tw1r": np.cos(2 * np.pi * k / 1024).astype(f), "tw1i": (-np.sin(2 * np.pi * k / 1024)).astype(f),
            "tw2r": np.cos(2 * np.pi * k2 / 2048).astype(f), "tw2i": (-np.sin(2 * np.pi * k2 / 2048)).astype(f),
            "hann": (0.5 - 0.5 * np.cos(2 * np.pi * i / 2048)).astype(f)}


def emulate_stft(wave, tb=None):
    """stft_kernel<false> of csrc/fft.hip in numpy float32, one operation per kernel operation: [R, n] -> [R, 2050, T]."""
    tb = kernel_tables() if tb is None else tb
    w = np.ascontiguousarray(wave, np.float32)
    R, n = w.shape
    T = frames_of(n)
    idx = np.abs(np.arange(T)[:, None] * HOP + np.arange(NFFT)[None, :] - NFFT // 2)        # sample2: reflect at 0 ...
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)                                         # ... and at n - 1
    fr = (w[:, idx] * tb["hann"]).reshape(R * T, NFFT)                                       # raw * win
    sr, si = np.ascontiguousarray(fr[:, 0::2]), np.ascontiguousarray(fr[:, 1::2])           # z = x[2c] + i x[2c + 1]
    tid = np.arange(256)
    for q in range(5):                                                                       # fft1024<false>
        p = 4 ** q
        k = tid & (p - 1)
        jo = ((tid - k) << 2) + k
        ur, ui = [sr[:, tid + 256 * m] for m in range(4)], [si[:, tid + 256 * m] for m in range(4)]
        if q > 0:
            for m in range(1, 4):
                tr, ti = tb["tw1r"][m * k * (256 // p)], tb["tw1i"][m * k * (256 // p)]
                ur[m], ui[m] = ur[m] * tr - ui[m] * ti, ur[m] * ti + ui[m] * tr             # cmul(u, t)
        v0r, v0i, v1r, v1i = ur[0] + ur[2], ui[0] + ui[2], ur[0] - ur[2], ui[0] - ui[2]
        v2r, v2i, dr, di = ur[1] + ur[3], ui[1] + ui[3], ur[1] - ur[3], ui[1] - ui[3]
        v3r, v3i = di, -dr                                                                   # -i * d
        nr, ni = np.empty_like(sr), np.empty_like(si)
        nr[:, jo], ni[:, jo] = v0r + v2r, v0i + v2i
        nr[:, jo + p], ni[:, jo + p] = v1r + v3r, v1i + v3i
        nr[:, jo + 2 * p], ni[:, jo + 2 * p] = v0r - v2r, v0i - v2i
        nr[:, jo + 3 * p], ni[:, jo + 3 * p] = v1r - v3r, v1i - v3i
        sr, si = nr, ni
    kk = np.arange(NBINS)                                                                    # rfft_split_store
    a, b, half = kk & 1023, (1024 - kk) & 1023, np.float32(0.5)
    zkr, zki, zcr, zci = sr[:, a], si[:, a], sr[:, b], -si[:, b]
    er, ei = half * (zkr + zcr), half * (zki + zci)
    orr, oi = half * (zki - zci), -half * (zkr - zcr)                                        # (zk - zc) / (2 i)
    xr = er + (tb["tw2r"] * orr - tb["tw2i"] * oi)
    xi = ei + (tb["tw2r"] * oi + tb["tw2i"] * orr)
    xi[:, [0, NBINS - 1]] = 0                                                                # exactly real for real input
    out = np.empty((R * T, F2), np.float32)
    out[:, 0::2], out[:, 1::2] = xr, xi
    assert out.dtype == xr.dtype == np.float32
    return np.ascontiguousarray(out.reshape(R, T, F2).transpose(0, 2, 1))


# ------------------------------------------------------------------------------------------ tests
def test_case_list_names_every_size():
    """The GPU file runs this list whole (it may skip no case); here: every (R, T) the kernels' edges need is in it."""
    assert sorted((R, frames_of(n)) for R, n in STFT_CASES) == sorted([
        (1, 2), (3, 2), (2, 3), (1, 5), (3, 9), (3, 31), (3, 32), (3, 33), (2, 34), (2, 127), (3, 128), (3, 129), (80, 125)])
    ns = [n for _, n in STFT_CASES]
    assert 1025 in ns and any(n % HOP == 0 for n in ns) and any(n % HOP == HOP - 1 for n in ns)
    runs = stft_runs()
    assert len(runs) == len(STFT_CASES) + 4 and len(set(runs)) == len(runs)
    assert {s for R, n, s in runs if (R, n) == SIGNAL_CASE} == set(SIGNALS)
    assert istft_shapes() == [(R, frames_of(n)) for R, n in STFT_CASES]
    assert BACKWARD_CASES == [(1, 2), (3, 5), (2, 9), (3, 33)]
    # the seeds give distinct inputs per case, and the same input twice
    assert np.array_equal(waveform(3, 2047), waveform(3, 2047)) and not np.array_equal(waveform(3, 2047)[0], waveform(3, 2047)[1])
    y = spectrum(2, 3)
    assert float(np.abs(y[:, 1, :]).min()) > 0 and float(np.abs(y[:, 2049, :]).min()) > 0


def test_kernel_tables_are_the_windows_and_twiddles_of_the_reference():
    tb = kernel_tables()
    assert np.abs(tb["hann"].astype(np.float64) - torch.hann_window(NFFT, dtype=torch.float64).numpy()).max() <= 2.0 ** -24
    assert tb["tw1r"][0] == 1 and tb["tw1i"][0] == 0 and tb["tw2r"][1024] == -1 and abs(tb["tw2i"][1024]) < 1e-15


@pytest.mark.parametrize("R,n,signal", stft_runs())
def test_float32_radix4_evaluation_meets_the_criterion(R, n, signal):
    wave = waveform(R, n, signal)
    x = emulate_stft(wave)
    assert x.shape == (R, F2, frames_of(n)) and x.dtype == np.float32
    assert not x[:, 1, :].any() and not x[:, 2049, :].any()
    hold("emulation R=%d n=%d %s" % (R, n, signal), x, ref_stft(wave, torch.float32), ref_stft(wave, torch.float64), per="frame")


def test_criterion_rejects_a_coarse_twiddle():
    """The bound has teeth: the same evaluation with one 2048-point twiddle rounded to bfloat16 misses it - in the max-abs form
    (two bins per frame are wrong; a frame's L2 norm over 1025 bins hardly moves, which is why both forms are asserted)."""
    tb = kernel_tables()
    for key in ("tw2r", "tw2i"):
        v = tb[key].copy()
        v[1] = torch.tensor(float(v[1])).to(torch.bfloat16).float().item()
        tb[key] = v
    R, n = 3, 2047
    wave = waveform(R, n)
    m = measure("emulation, tw2048[1] in bfloat16", emulate_stft(wave, tb), ref_stft(wave, torch.float32), ref_stft(wave, torch.float64),
                per="frame")
    assert m["e"] > m["bound"]
