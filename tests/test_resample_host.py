"""CPU-side tests of the sample-rate conversion (bsrnn_resample, bsrnn_resampler_*): the definition in csrc/resample_host.h - taps, lengths,
index ranges, the closed form, the polyphase table, ready() - against scipy.signal in float64 and against Python's integers (through the small
program tests/cpp/resample_check.cpp, built with -Wall -Werror and a second time with the address and undefined-behaviour sanitizers), the
declarations, exports and bindings, argument checking on a host-only context, and the Python layer's signatures and shape errors.  No compute
here; tests/test_gpu_resample.py holds the kernel."""
import ctypes
import inspect
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest
from scipy import signal

from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "resample_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
PAIRS = [(48000, 44100), (44100, 48000), (16000, 44100), (192000, 44100), (22050, 44100), (44100, 22050), (44100, 44100)]
SIZES = [1, 5, 1023, 1024, 20000]
NEW = ["bsrnn_resample_len", "bsrnn_resample", "bsrnn_resampler_create", "bsrnn_resampler_destroy", "bsrnn_resampler_reset",
       "bsrnn_resampler_ready", "bsrnn_resampler_process", "bsrnn_resampler_flush"]


def reduced(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    return up, down, 10 * max(up, down)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output lines."""
    exe = str(tmp_path_factory.mktemp("resample") / "resample_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["resample_host.h"]          # the host header only
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")[:-1]
    return run


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


# ------------------------------------------------------------------------------------------------ resample_host.h
def test_self_checks_under_the_sanitizers(check, tmp_path):
    """The table holds every tap once and zeros elsewhere, the polyphase form is the closed form, ready() and the carry bound over random
    block splits: the program's own checks, run plain and under -fsanitize=address,undefined."""
    assert check("self") == ["ok"]
    exe = str(tmp_path / "resample_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


@pytest.mark.parametrize("pair", PAIRS)
def test_taps_against_firwin(check, pair):
    up, down, half = reduced(*pair)
    lines = check("taps", *pair)
    assert [int(v) for v in lines[0].split()][:3] == [up, down, half]
    h = np.array([float(v) for v in lines[1:]])
    assert h.shape == (2 * half + 1,)
    if up == down:
        # scipy's firwin refuses a cutoff AT Nyquist (resample_poly returns a copy before it designs anything); the formula's value there is
        # the unit impulse, which is what makes the conversion a copy
        ref = np.zeros(21)
        ref[10] = 1.0
    else:
        ref = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    err = float(np.abs(h - ref).max())
    print("taps %s: max |h - firwin| = %.3e" % (pair, err))
    assert err <= 1e-12
    # also tap by tap, far below fp32 rounding: the taps at multiples of max(up, down) are about 1e-17 in firwin, not zero, and a signal
    # that meets only those (an impulse, in the GPU test) must still agree with resample_poly to the fp32 bound.
    # DEPENDENCY: for the taps above 1e-12 of the peak this is mathematics.  For the ones below - rounding residue of sin() near a multiple
    # of pi - it holds only while this libm's sin() and numpy's give the same value, to a few ulp, for the same rounded argument; the
    # 1e-12 absolute check above does not see them.  The two parts are reported apart: if only the second one moves after a change of
    # scipy, numpy or libm, the design is not at fault, and the impulse row of tests/test_gpu_resample.py will move with it.
    nz = ref != 0
    big = np.abs(ref) >= 1e-12 * np.abs(ref).max()
    rel = np.zeros_like(ref)
    rel[nz] = np.abs(h - ref)[nz] / np.abs(ref[nz])
    rel_big, rel_small = float(rel[big].max()), float(rel[nz & ~big].max()) if (nz & ~big).any() else 0.0
    print("taps %s: max relative difference = %.3e above 1e-12 of the peak, %.3e below (%d taps)" % (pair, rel_big, rel_small, (nz & ~big).sum()))
    assert rel_big <= 1e-10
    assert rel_small <= 1e-10, "the taps firwin leaves at about 1e-17 differ: sin() of this libm against numpy's, not the design (see above)"
    assert np.array_equal(h == 0, ref == 0)
    # rounding to fp32 happens once, in the table: the header's table rows are float32(h)
    kh, L = [int(v) for v in lines[0].split()][3:]
    assert kh == half // up and L == kh + (half + up - 1) // up + 1


@pytest.mark.parametrize("pair", PAIRS)
def test_lengths_and_index_ranges(check, pair):
    up, down, half = reduced(*pair)
    for n in SIZES:
        lines = check("ranges", *pair, n)
        n_out = -(-n * up // down)
        assert int(lines[0]) == n_out == len(signal.resample_poly(np.zeros(n), up, down))
        got = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], dtype=np.int64).reshape(n_out, 2)
        c = np.arange(n_out, dtype=np.int64) * down
        first = np.maximum(0, -((half - c) // up))          # ceil((c - half) / up)
        last = np.minimum(n - 1, (c + half) // up)
        assert np.array_equal(got[:, 0], first) and np.array_equal(got[:, 1], last)


@pytest.mark.parametrize("pair", PAIRS)
def test_closed_form_against_resample_poly(check, pair, tmp_path):
    up, down, _ = reduced(*pair)
    rng = np.random.default_rng(3)
    for n in (1, 5, 1023, 3000):
        x = rng.standard_normal(n)
        x[-1] = 1.0
        f = tmp_path / ("x%d.f64" % n)
        x.tofile(f)
        y = np.array([float(v) for v in check("apply", *pair, f)])
        ref = signal.resample_poly(x, up, down)
        assert y.shape == ref.shape
        err = float(np.abs(y - ref).max())
        print("closed form %s n = %d: max |y - resample_poly| = %.3e" % (pair, n, err))
        assert err < 1e-12


@pytest.mark.parametrize("pair", PAIRS)
def test_ready_against_a_count(check, pair):
    up, down, half = reduced(*pair)
    rnd = random.Random(5)
    for n in SIZES:
        # cumulative lengths of a random split, zero-length blocks included
        cuts, N = [0], 0
        while N < n:
            N = min(n, N + (0 if rnd.random() < 0.25 else rnd.randrange(0, n // 3 + 2)))
            cuts.append(N)
        got = [int(v) for v in check("ready", *pair, *cuts)]
        n_out = -(-n * up // down)
        want = [min(-(-N * up // down), sum(1 for j in range(-(-N * up // down)) if (j * down + half) // up <= N - 1)) for N in cuts]
        assert got == want
        assert all(b >= a for a, b in zip(got, got[1:])) and got[-1] <= n_out
        counts = [b - a for a, b in zip(got, got[1:])]
        assert sum(counts) + (n_out - got[-1]) == n_out


def test_index_helpers_beyond_32_bits(check):
    """j near 2^40 (j * down near 2^50): the 64-bit path no small GPU shape reaches, against Python's integers."""
    rnd = random.Random(9)
    for pair in PAIRS + [(1, 1024), (1024, 1)]:
        up, down, half = reduced(*pair)
        for _ in range(6):
            j = (1 << 40) + rnd.randrange(-5000, 5000)
            n_in = -(-j * down // up) + rnd.randrange(-3, 40)
            got = [int(v) for v in check("index", up, down, half, n_in, j)[0].split()]
            c = j * down
            ready = min(-(-j * up // down), max(0, (j * up - half - 1) // down + 1))
            assert got == [max(0, -((half - c) // up)), min(n_in - 1, (c + half) // up), c % up, c // up - half // up, -(-j * up // down), ready]


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {
        "bsrnn_resample_len": ("int64_t", ["int64_t", "int32_t", "int32_t"]),
        "bsrnn_resample": ("int", ["bsrnn_ctx*", "constfloat*", "int64_t", "float*", "int64_t", "int32_t", "int64_t", "int32_t", "int32_t", "void*"]),
        "bsrnn_resampler_create": ("int", ["bsrnn_ctx*", "int32_t", "int32_t", "int32_t", "bsrnn_resampler**"]),
        "bsrnn_resampler_destroy": ("void", ["bsrnn_resampler*"]),
        "bsrnn_resampler_reset": ("int", ["bsrnn_resampler*", "void*"]),
        "bsrnn_resampler_ready": ("int64_t", ["constbsrnn_resampler*", "int64_t"]),
        "bsrnn_resampler_process": ("int", ["bsrnn_resampler*", "constfloat*", "int64_t", "int64_t", "float*", "int64_t", "int64_t*", "void*"]),
        "bsrnn_resampler_flush": ("int", ["bsrnn_resampler*", "float*", "int64_t", "int64_t*", "void*"]),
    }
    for name, (ret, types) in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, body, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, name
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body)
    # the documentation says what the calls replace and what is not pinned
    assert "infer-streaming.py:77-78" in txt and "resample_poly" in txt and re.search(r"ffmpeg.{0,80}NOT pinned", txt, flags=re.S)


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_resample.argtypes == [vp, vp, i64, vp, i64, i32, i64, i32, i32, vp]
    assert native.lib.bsrnn_resample_len.restype == i64 and native.lib.bsrnn_resampler_ready.restype == i64
    assert native.lib.bsrnn_resampler_process.argtypes == [vp, vp, i64, i64, vp, i64, ctypes.POINTER(i64), vp]
    assert native.lib.bsrnn_abi_version() == 2


def test_resample_len_needs_no_context(native):
    f = native.lib.bsrnn_resample_len
    for rate_in, rate_out in PAIRS:
        up, down, _ = reduced(rate_in, rate_out)
        for n in SIZES + [(1 << 40) + 1]:
            assert f(n, rate_in, rate_out) == -(-n * up // down)
    assert f(0, 48000, 44100) == -1 and f(-5, 48000, 44100) == -1
    assert f(100, 0, 44100) == -1 and f(100, 44100, -1) == -1
    assert f(100, 44100, 48001) == -1                       # reduces to 48001 / 44100
    assert f(100, 2048, 2) == 100 // 1024 + 1 and f(100, 2050, 2) == -1


def test_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib
    a, b = np.zeros((3, 100), np.float32), np.zeros((3, 100), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)

    def err():
        return lib.bsrnn_last_error().decode()
    call = lib.bsrnn_resample
    assert call(None, pa, 100, pb, 100, 3, 100, 48000, 44100, None) == EARG
    assert call(host_ctx, None, 100, pb, 100, 3, 100, 48000, 44100, None) == EARG
    assert call(host_ctx, pa, 100, None, 100, 3, 100, 48000, 44100, None) == EARG
    assert call(host_ctx, pa, 100, pb, 100, 0, 100, 48000, 44100, None) == EARG
    # every limit, each with a text that names the value
    assert call(host_ctx, pa, 100, pb, 100, 3, 100, 0, 44100, None) == EARG
    assert "rate_in = 0" in err(), err()
    assert call(host_ctx, pa, 100, pb, 100, 3, 100, 48000, -7, None) == EARG
    assert "rate_out = -7" in err(), err()
    assert call(host_ctx, pa, 100, pb, 100, 3, 100, 44100, 48001, None) == EARG
    assert "48001 / 44100" in err() and "1024" in err(), err()
    assert call(host_ctx, pa, 100, pb, 100, 3, 100, 1025, 1, None) == EARG
    assert "1 / 1025" in err(), err()
    assert call(host_ctx, pa, 100, pb, 100, 3, 0, 48000, 44100, None) == EARG
    assert re.search(r"n_in >= 1\b.* 0\b", err()), err()
    assert call(host_ctx, pa, 100, pb, 100, 3, -4, 48000, 44100, None) == EARG
    assert "-4" in err(), err()
    # a stride shorter than its row; the output over the input
    assert call(host_ctx, pa, 99, pb, 100, 3, 100, 48000, 44100, None) == EARG
    assert "in_stride 99" in err(), err()
    assert call(host_ctx, pa, 100, pb, 91, 3, 100, 48000, 44100, None) == EARG          # ceil(100 * 147 / 160) = 92
    assert "out_stride 91" in err() and "92" in err(), err()
    assert call(host_ctx, pa, 100, pa, 100, 3, 100, 48000, 44100, None) == EARG
    assert "overlap" in err(), err()
    tail = ctypes.c_void_p(pa.value + 4 * 299)                                          # the last float of the input block
    assert call(host_ctx, pa, 100, tail, 100, 3, 100, 44100, 44100, None) == EARG
    assert "overlap" in err(), err()
    # valid arguments (equal rates too): a host-only context cannot compute
    for rates in ((48000, 44100), (44100, 44100), (192000, 44100)):
        assert call(host_ctx, pa, 100, pb, 100, 3, 100, rates[0], rates[1], None) == ESTATE
        assert "host-only" in err(), err()
    assert not a.any() and not b.any()
    # the streaming object: the same limits in front of the same BSRNN_ESTATE
    rs = ctypes.c_void_p()
    make = lib.bsrnn_resampler_create
    assert make(None, 2, 48000, 44100, ctypes.byref(rs)) == EARG
    assert make(host_ctx, 0, 48000, 44100, ctypes.byref(rs)) == EARG
    assert "C = 0" in err(), err()
    assert make(host_ctx, 2, 48000, 44100, None) == EARG
    assert make(host_ctx, 2, 0, 44100, ctypes.byref(rs)) == EARG
    assert "rate_in = 0" in err(), err()
    assert make(host_ctx, 2, 44100, 48001, ctypes.byref(rs)) == EARG
    assert "48001 / 44100" in err(), err()
    assert make(host_ctx, 2, 48000, 44100, ctypes.byref(rs)) == ESTATE
    assert not rs.value
    # null objects
    n = ctypes.c_int64(-5)
    assert lib.bsrnn_resampler_process(None, pa, 100, 10, pb, 100, ctypes.byref(n), None) == EARG
    assert lib.bsrnn_resampler_flush(None, pb, 100, ctypes.byref(n), None) == EARG
    assert lib.bsrnn_resampler_reset(None, None) == EARG
    assert lib.bsrnn_resampler_ready(None, 10) == -1 and n.value == -5
    lib.bsrnn_resampler_destroy(None)


# ------------------------------------------------------------------------------------------------ Python layer
def test_python_layer_signatures_and_shape_errors(native):
    import torch
    from speechseparation_amd import bsrnn
    from speechseparation_amd.bsrnn import BSRNN, Resampler
    sig = inspect.signature(BSRNN.resample)
    assert list(sig.parameters) == ["self", "wave", "rate_in", "rate_out", "out"] and sig.parameters["out"].default is None
    sig = inspect.signature(BSRNN.separate_at_rate)
    assert list(sig.parameters) == ["self", "wave", "sample_rate", "model_rate", "segment_frames"]
    assert sig.parameters["model_rate"].default == 44100 and sig.parameters["segment_frames"].default is None
    assert list(inspect.signature(Resampler.__init__).parameters) == ["self", "model", "channels", "rate_in", "rate_out"]
    for name in ("ready", "process", "flush", "reset"):
        assert callable(getattr(Resampler, name))
    assert bsrnn.resample_len(480, 48000, 44100) == 441 and bsrnn.resample_len(1, 16000, 44100) == 3
    m = BSRNN()
    w = torch.zeros((2, 480))
    for bad in (lambda: m.resample(torch.zeros(480), 48000, 44100),                      # not [R, n]
                lambda: m.resample(torch.zeros((2, 0)), 48000, 44100),                   # no samples
                lambda: m.resample(w, 0, 44100),
                lambda: m.resample(w, 44100, 48001),                                     # reduces beyond 1024
                lambda: m.resample(w, 48000, 44100, out=torch.zeros((2, 440))),          # 441 samples come out
                lambda: m.resample(w.double(), 48000, 44100),
                lambda: m.separate_at_rate(torch.zeros(480), 48000),
                lambda: m.separate_at_rate(w, 0),
                lambda: m.separate_at_rate(w, 48000, segment_frames=0),
                lambda: bsrnn.resample_len(0, 48000, 44100)):
        with pytest.raises(ValueError):
            bad()
    assert m._ctx is None


def test_entry_points_have_the_options():
    assert re.search(r'add_argument\("--model-rate", type=int, default=0', open(os.path.join(REPO, "infer.py")).read())
    assert re.search(r'add_argument\("--device-resample", action="store_true"', open(os.path.join(REPO, "infer-streaming.py")).read())
