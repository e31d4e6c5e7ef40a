"""The critic's 4096-point analysis (bsrnn_critic_spectrum; csrc/critic_spectrum_host.h, csrc/stft4096.hip) without a GPU: the case table
and the references the GPU file shares, a numpy float32 restatement of the kernel's arithmetic held to the project's criterion
(tests/test_dsp_reference.py: e <= 3 e_f32 + 2^-24 max|ref64|, max-abs and L2 per frame) on every case, the host header through the small
program tests/cpp/critic_spectrum_check.cpp (plain and under the address and undefined-behaviour sanitizers), the declarations, bindings
and exports, and the argument refusals on a host-only context.

The reference is the reference's own call (train-discriminator.py:62-68): torch.stft(w, n_fft=4096, hop_length=1024,
window=hann_window(4096)) - centred, reflect padding - then cat(real, imag), in float64 (ref64) and in float32 (ref32) on the CPU."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from test_dsp_reference import SIGNALS, hold, waveform

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "critic_spectrum_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
NFFT, HOP, BINS, CH = 4096, 1024, 2049, 4098
# the edges critic_spectrum_host.h names: frames per workgroup, frames x bins of a transpose tile, rows x frames the scratch holds
CHUNK, TILE_T, TILE_B, CAP_UNITS = 4, 32, 64, 128
NEW = ["bsrnn_critic_spectrum", "bsrnn_critic_spectrum_layout"]

# (R, n): T = 1 + n // 1024.  The first nine are the issue's; the rest sit just below, at and just past the edges of the kernels
CASES = [
    (1, 2049),                 # T 3: the minimum; a frame reflected at both ends; one frame short of a chunk
    (3, 4095),                 # T 4: n % 1024 = 1023; exactly one chunk
    (2, 4096),                 # T 5: a chunk and a one-frame tail (dummy reload)
    (1, 3 * 1024 + 1),         # T 4: short clip, odd n
    (3, 8 * 1024 + 1023),      # T 9: runs all five SIGNALS
    (2, 33 * 1024 + 1),        # T 34: not a multiple of 4, rows of x not 16-byte aligned
    (3, 64 * 1024 + 9),        # T 65: odd; two transpose tiles and one frame
    (2, 600 * 1024),           # T 601: the critic's shortest input
    (80, 20 * 1024 + 500),     # T 21, 80 rows: 32 frames per slab, 480 workgroups
    (2, 30 * 1024 + 5),        # T 31: one frame short of a transpose tile
    (2, 31 * 1024),            # T 32: a whole tile
    (2, 32 * 1024 + 77),       # T 33: a tile and one frame
    (128, 30 * 1024 + 3),      # T 31, 128 rows (32 frames per slab): one frame short of the slab
    (128, 31 * 1024 + 1),      # T 32: the slab exactly, 1024 workgroups
    (128, 32 * 1024 + 9),      # T 33: a second slab of one frame
    (127, 2049 + 40),          # one row short of a row block
    (129, 2 * 1024 + 700),     # a second row block of one row
]
SIGNAL_CASE = (3, 8 * 1024 + 1023)


def frames_of(n):
    return 1 + n // HOP


def runs():
    """(R, n, signal) of every run, in a fixed order."""
    return [(R, n, "gaussian") for R, n in CASES] + [SIGNAL_CASE + (s,) for s in SIGNALS[1:]]


def ref_spectrum(wave, dtype):
    """[R, n] float32 -> [R, 4098, T] in `dtype`, as train-discriminator.py:62-68 forms it."""
    w = torch.from_numpy(np.ascontiguousarray(wave, np.float32)).to(dtype)
    X = torch.stft(w, n_fft=NFFT, hop_length=HOP, window=torch.hann_window(NFFT, dtype=dtype), center=True, pad_mode="reflect",
                   return_complex=True)
    return torch.cat((X.real, X.imag), dim=1).numpy()


_REFS = {}


def references(R, n, signal="gaussian"):
    """(wave, ref32, ref64) of a run, computed once and shared (treat as read-only)."""
    key = (R, n, signal)
    if key not in _REFS:
        w = waveform(R, n, signal)
        _REFS[key] = (w, ref_spectrum(w, torch.float32), ref_spectrum(w, torch.float64))
    return _REFS[key]


# ------------------------------------------------------------------------------------------ the kernel's arithmetic
def kernel_tables():
    """The tables api_critic.hip builds at the first call: evaluated in double, rounded to float."""
    k, k2, i, f = np.arange(2048, dtype=np.float64), np.arange(BINS, dtype=np.float64), np.arange(NFFT, dtype=np.float64), np.float32
    return {"twr": np.cos(2 * np.pi * k / 2048).astype(f), "twi": (-np.sin(2 * np.pi * k / 2048)).astype(f),
            "spr": np.cos(2 * np.pi * k2 / NFFT).astype(f), "spi": (-np.sin(2 * np.pi * k2 / NFFT)).astype(f),
            "hann": (0.5 - 0.5 * np.cos(2 * np.pi * i / NFFT)).astype(f)}


def emulate(wave, scale=1.0, tb=None):
    """spectrum4096_kernel + spectrum_transpose_kernel of csrc/stft4096.hip in numpy float32, one operation per kernel operation:
    [R, n] -> [R, 4098, T]."""
    tb = kernel_tables() if tb is None else tb
    w = np.ascontiguousarray(wave, np.float32)
    R, n = w.shape
    T = frames_of(n)
    idx = np.abs(np.arange(T)[:, None] * HOP + np.arange(NFFT)[None, :] - NFFT // 2)        # scaled_sample2: reflect at 0 ...
    idx = np.where(idx >= n, 2 * (n - 1) - idx, idx)                                         # ... and at n - 1
    fr = ((w[:, idx] * np.float32(scale)) * tb["hann"]).reshape(R * T, NFFT)                 # (raw * scale) * win
    ar, ai = fr[:, 0::2], fr[:, 1::2]                                                        # z[c] = x[2c] + i x[2c + 1]
    sr, si = np.empty_like(ar), np.empty_like(ai)                                            # radix 2 on (c, c + 1024) -> points 2c, 2c + 1
    sr[:, 0::2], sr[:, 1::2] = ar[:, :1024] + ar[:, 1024:], ar[:, :1024] - ar[:, 1024:]
    si[:, 0::2], si[:, 1::2] = ai[:, :1024] + ai[:, 1024:], ai[:, :1024] - ai[:, 1024:]
    j = np.arange(512)
    for p in (2, 8, 32, 128, 512):                                                           # pass4<P>
        k = j & (p - 1)
        jo = ((j - k) << 2) + k
        ur, ui = [sr[:, j + 512 * m] for m in range(4)], [si[:, j + 512 * m] for m in range(4)]
        for m in range(1, 4):
            tr, ti = tb["twr"][m * k * (512 // p)], tb["twi"][m * k * (512 // p)]
            ur[m], ui[m] = ur[m] * tr - ui[m] * ti, ur[m] * ti + ui[m] * tr                 # cmul(u, t)
        v0r, v0i, v1r, v1i = ur[0] + ur[2], ui[0] + ui[2], ur[0] - ur[2], ui[0] - ui[2]
        v2r, v2i, dr, di = ur[1] + ur[3], ui[1] + ui[3], ur[1] - ur[3], ui[1] - ui[3]
        v3r, v3i = di, -dr                                                                   # -i * d
        nr, ni = np.empty_like(sr), np.empty_like(si)
        nr[:, jo], ni[:, jo] = v0r + v2r, v0i + v2i
        nr[:, jo + p], ni[:, jo + p] = v1r + v3r, v1i + v3i
        nr[:, jo + 2 * p], ni[:, jo + 2 * p] = v0r - v2r, v0i - v2i
        nr[:, jo + 3 * p], ni[:, jo + 3 * p] = v1r - v3r, v1i - v3i
        sr, si = nr, ni
    kk = np.arange(BINS)                                                                     # the real split
    a, b, half = kk & 2047, (2048 - kk) & 2047, np.float32(0.5)
    zkr, zki, zcr, zci = sr[:, a], si[:, a], sr[:, b], -si[:, b]
    er, ei = half * (zkr + zcr), half * (zki + zci)
    orr, oi = half * (zki - zci), -half * (zkr - zcr)                                        # (zk - zc) / (2 i)
    xr = er + (tb["spr"] * orr - tb["spi"] * oi)
    xi = ei + (tb["spr"] * oi + tb["spi"] * orr)
    xi[:, [0, BINS - 1]] = 0                                                                 # exactly real for real input
    assert xr.dtype == xi.dtype == np.float32
    out = np.concatenate((xr.reshape(R, T, BINS), xi.reshape(R, T, BINS)), axis=2)          # the transpose: re rows, then im rows
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def test_case_table_names_every_edge():
    have = sorted((R, frames_of(n)) for R, n in CASES)
    assert have == sorted([(1, 3), (3, 4), (2, 5), (1, 4), (3, 9), (2, 34), (3, 65), (2, 601), (80, 21), (2, 31), (2, 32), (2, 33),
                           (128, 31), (128, 32), (128, 33), (127, 3), (129, 3)])
    ts = {T for _, T in have}
    assert {CHUNK - 1, CHUNK, CHUNK + 1} <= ts and {TILE_T - 1, TILE_T, TILE_T + 1} <= ts
    slab = TILE_T * (CAP_UNITS // 128)                                     # frames per slab at 128 rows
    assert {(128, slab - 1), (128, slab), (128, slab + 1)} <= set(have)
    assert {R for R, _ in have} >= {CAP_UNITS - 1, CAP_UNITS, CAP_UNITS + 1}
    assert all(n > 2048 for _, n in CASES) and any(n % HOP == HOP - 1 for _, n in CASES) and any(n % HOP == 0 for _, n in CASES)
    assert len(set(runs())) == len(runs()) == len(CASES) + 4


def test_tables_are_the_window_and_twiddles_of_the_reference():
    tb = kernel_tables()
    assert np.abs(tb["hann"].astype(np.float64) - torch.hann_window(NFFT, dtype=torch.float64).numpy()).max() <= 2.0 ** -24
    assert tb["twr"][0] == 1 and tb["twi"][0] == 0 and tb["twi"][512] == -1 and tb["spr"][2048] == -1 and abs(tb["spi"][2048]) < 1e-15


@pytest.mark.parametrize("R,n,signal", runs())
def test_float32_restatement_meets_the_criterion(R, n, signal):
    wave, ref32, ref64 = references(R, n, signal)
    x = emulate(wave)
    assert x.shape == (R, CH, frames_of(n)) and x.dtype == np.float32
    assert not x[:, BINS, :].any() and not x[:, CH - 1, :].any()
    hold("restatement R=%d n=%d %s" % (R, n, signal), x, ref32, ref64, per="frame")


def test_restatement_with_a_scale():
    R, n = 2, 5 * 1024 + 3
    wave = waveform(R, n)
    scaled = wave * np.float32(0.37)
    assert np.array_equal(emulate(wave, 0.37), emulate(scaled, 1.0))
    hold("restatement, scale 0.37", emulate(wave, 0.37), ref_spectrum(scaled, torch.float32), ref_spectrum(scaled, torch.float64), per="frame")


# ------------------------------------------------------------------------------------------ critic_spectrum_host.h
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output."""
    exe = str(tmp_path_factory.mktemp("critic_spectrum") / "critic_spectrum_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["critic_spectrum_host.h"]          # the host header only
    assert not re.search(r"#include\s+[<\"]hip", open(os.path.join(CSRC, "critic_spectrum_host.h")).read())
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout
    return run


def test_self_checks_under_the_sanitizers(check, tmp_path):
    assert check("self").strip() == "ok"
    exe = str(tmp_path / "critic_spectrum_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_frames_and_reflected_indices(check):
    for n in (2049, 2050, 3071, 3072, 4095, 4096, 5000, 614400):
        T = int(check("frames", n))
        assert T == frames_of(n) == ref_spectrum(np.zeros((1, n), np.float32), torch.float32).shape[2]
        padded = np.pad(np.arange(n), NFFT // 2, mode="reflect")
        for t in sorted({0, 1, 2, T - 2, T - 1}):
            got = np.array(check("reflect", n, t).split(), dtype=np.int64)
            assert got.shape == (NFFT,) and np.array_equal(got, padded[t * HOP:t * HOP + NFFT]), (n, t)
    # the minimum length: frame 1 of n = 2049 is reflected at both ends
    got = np.array(check("reflect", 2049, 1).split(), dtype=np.int64)
    assert got[0] == 1024 and got[1024] == 0 and got[-1] == 2 * 2048 - 3071


PLAN_SHAPES = [(R, n) for R in (1, 2, 4, 63, 64, 65, 80, 127, 128, 129, 300) for n in (2049, 4096, 32 * 1024 + 9, 614400, 2646000)
               if R * CH * frames_of(n) < 2 ** 31]


@pytest.mark.parametrize("shape", PLAN_SHAPES, ids=lambda s: "%d-%d" % s)
def test_slabs_cover_every_frame_exactly_once(check, shape):
    R, n = shape
    g = json.loads(check("plan", R, n))
    T = frames_of(n)
    assert (g["chunk"], g["tile_t"], g["tile_b"], g["cap_units"], g["channels"]) == (CHUNK, TILE_T, TILE_B, CAP_UNITS, CH)
    assert g["T"] == T and g["rows_per_block"] == min(R, CAP_UNITS) and g["row_blocks"] == -(-R // g["rows_per_block"])
    assert g["frames_per_slab"] == TILE_T * (CAP_UNITS // g["rows_per_block"]) and g["frame_slabs"] == -(-T // g["frames_per_slab"])
    assert g["slabs"] == g["row_blocks"] * g["frame_slabs"] == len(g["list"])
    assert g["scratch_floats"] == g["rows_per_block"] * min(T, g["frames_per_slab"]) * CH <= CAP_UNITS * TILE_T * CH
    seen = np.zeros((R, T), np.int32)
    for r0, r1, t0, t1 in g["list"]:
        assert 0 <= r0 < r1 <= R and 0 <= t0 < t1 <= T and t0 % g["frames_per_slab"] == 0 and r0 % g["rows_per_block"] == 0
        assert (r1 - r0) * (t1 - t0) * CH <= g["scratch_floats"]
        seen[r0:r1, t0:t1] += 1
    assert (seen == 1).all()
    assert json.loads(check("plan", R, n)) == g                          # a function of the shape only


def test_refusals_of_the_header(check):
    ok = lambda *a: int(check("check", *a))       # noqa: E731
    assert ok(1, 2049, 2049, 1) == 0 and ok(4, 614400, 700000, 0.02) == 0 and ok(3, 4096, 4096, 0) == 0 and ok(3, 4096, 4096, -2.5) == 0
    assert ok(0, 4096, 4096, 1) == 1 and ok(-3, 4096, 4096, 1) == 1
    assert ok(2, 2048, 2048, 1) == 2 and ok(2, 0, 0, 1) == 2 and ok(2, -5, 10, 1) == 2
    assert ok(2, 4096, 4095, 1) == 3
    assert ok(2, 4096, 4096, "inf") == 4 and ok(2, 4096, 4096, "-inf") == 4 and ok(2, 4096, 4096, "nan") == 4
    # R * 4098 * T against 2^31 - 1: 174 762 * 4098 * 3 = 2 148 524 028 is past it, one row less is not
    assert ok(174762, 2049, 2049, 1) == 5 and ok(174677, 2049, 2049, 1) == 0 and ok(174678, 2049, 2049, 1) == 5
    assert ok(1, 1 << 40, 1 << 40, 1) == 5 and ok(1 << 33, 4096, 4096, 1) == 5
    # the order of the verdicts
    assert ok(0, 100, 50, "nan") == 1 and ok(2, 100, 50, "nan") == 2 and ok(2, 4096, 50, "nan") == 3


# ------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def native():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd import _native
    return _native


@pytest.fixture()
def host_ctx(native):
    from speechseparation_amd import spec
    v = spec.generate_bandsplits()[0]
    ctx = ctypes.c_void_p()
    assert native.lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(ctx)) == 0
    yield ctx
    native.lib.bsrnn_destroy(ctx)


def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {
        "bsrnn_critic_spectrum": ("int", ["bsrnn_ctx*", "constfloat*", "int64_t", "float*", "int32_t", "int64_t", "float", "void*"]),
        "bsrnn_critic_spectrum_layout": ("int", ["int32_t", "int64_t", "int64_t"]),
    }
    for name, (ret, types) in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, body, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*(\[\d+\])?$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, (name, got)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body)
    assert "train-discriminator.py:62-68" in txt and "hann_window(4096)" in txt


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_critic_spectrum.argtypes == [vp, vp, i64, vp, i32, i64, ctypes.c_float, vp]
    assert native.lib.bsrnn_critic_spectrum_layout.argtypes == [i32, i64, ctypes.POINTER(i64)]
    assert native.lib.bsrnn_abi_version() == 2


def test_layout_needs_no_context(native, check):
    f = native.lib.bsrnn_critic_spectrum_layout
    out = (ctypes.c_int64 * 4)()
    for R, n in [(1, 2049), (4, 614400), (4, 2646000), (80, 20 * 1024 + 500), (128, 32 * 1024 + 9), (129, 2748)]:
        g = json.loads(check("plan", R, n))
        assert f(R, n, out) == 0 and list(out) == [g["T"], g["slabs"], g["frames_per_slab"], g["scratch_floats"]]
    assert list(out) == [3, 2, 32, 128 * 3 * CH]
    assert f(4, 2646000, out) == 0 and list(out) == [2584, 3, 1024, 4 * 1024 * CH]     # a 60 s clip: 67 MB, not 169
    err = lambda: native.lib.bsrnn_last_error().decode()       # noqa: E731
    assert f(4, 614400, None) == EARG
    assert f(0, 614400, out) == EARG and "R = 0" in err()
    assert f(4, 2048, out) == EARG and "n = 2048" in err()
    assert f(174678, 2049, out) == EARG and "2^31" in err()


def test_argument_errors_without_a_device(native, host_ctx):
    call = native.lib.bsrnn_critic_spectrum
    w, x = np.zeros((3, 5000), np.float32), np.zeros((3, CH, 5), np.float32)
    pw, px = w.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)
    err = lambda: native.lib.bsrnn_last_error().decode()       # noqa: E731
    assert call(None, pw, 5000, px, 3, 4096, 1.0, None) == EARG and "null context" in err()
    assert call(host_ctx, None, 5000, px, 3, 4096, 1.0, None) == EARG and "null argument" in err()
    assert call(host_ctx, pw, 5000, None, 3, 4096, 1.0, None) == EARG and "null argument" in err()
    assert call(host_ctx, pw, 5000, px, 0, 4096, 1.0, None) == EARG and "R = 0" in err(), err()
    assert call(host_ctx, pw, 5000, px, 3, 2048, 1.0, None) == EARG and re.search(r"n > 2048\b.*n = 2048\b", err()), err()
    assert call(host_ctx, pw, 5000, px, 3, -1, 1.0, None) == EARG and "n = -1" in err(), err()
    assert call(host_ctx, pw, 4095, px, 3, 4096, 1.0, None) == EARG and "wave_stride 4095" in err() and "n = 4096" in err(), err()
    for bad in (float("inf"), float("-inf"), float("nan")):
        assert call(host_ctx, pw, 5000, px, 3, 4096, bad, None) == EARG and "scale" in err() and "finite" in err(), err()
    assert call(host_ctx, pw, 5000, px, 174678, 2049, 1.0, None) == EARG and "2^31" in err(), err()
    # valid arguments: a host-only context cannot compute
    assert call(host_ctx, pw, 5000, px, 3, 4096, 0.5, None) == ESTATE and "host-only" in err(), err()
    assert not w.any() and not x.any()


# ------------------------------------------------------------------------------------------ Python layer
def test_python_layer(native):
    from speechseparation_amd import discriminator
    sig = inspect.signature(discriminator.critic_spectrum)
    assert list(sig.parameters) == ["wave", "scale"] and sig.parameters["scale"].default == 1.0
    with pytest.raises(ValueError, match="cuda"):
        discriminator.critic_spectrum(torch.zeros(2, 4096))                  # no CPU fallback
    with pytest.raises(ValueError, match=r"\[R, n\]"):
        discriminator.critic_spectrum(torch.zeros(4096))
    assert discriminator.spectrum_layout(4, 2646000) == {"T": 2584, "slabs": 3, "frames_per_slab": 1024, "scratch_floats": 4 * 1024 * CH}
    assert "no 4096-point" not in open(os.path.join(REPO, "speechseparation_amd", "discriminator.py")).read()
    txt = open(os.path.join(REPO, "train-discriminator.py")).read()
    assert re.search(r'add_argument\("--n_fft", type=int, choices=\(2048, 4096\), default=2048', txt)
