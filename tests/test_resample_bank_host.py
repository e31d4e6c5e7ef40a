"""CPU-side tests of the resampler bank (bsrnn_resampler_bank_*, bsrnn.ResamplerBank, StreamPool(rates=...)): the per-row arithmetic of
csrc/resample_bank_host.h - every row against a single-pair stream of its pair, the descriptor's fields, the kernel's tile arithmetic, the
size of a group of descriptors - through the small program tests/cpp/resample_bank_check.cpp (built with -Wall -Werror and a second time
with the address and undefined-behaviour sanitizers), descriptor fields at stream positions near 2^40 against Python's integers, the
declarations and bindings, and every refusal that is answered before a device is touched.  No compute here; tests/test_gpu_resample_bank.py
and tests/test_gpu_stream_pool_rates.py hold the kernel and the pool."""
import ctypes
import inspect
import math
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "resample_bank_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
NEW = ["bsrnn_resampler_bank_create", "bsrnn_resampler_bank_destroy", "bsrnn_resampler_bank_assign", "bsrnn_resampler_bank_pair_of",
       "bsrnn_resampler_bank_ready", "bsrnn_resampler_bank_process", "bsrnn_resampler_bank_flush_rows", "bsrnn_resampler_bank_reset_rows"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output lines."""
    exe = str(tmp_path_factory.mktemp("resample_bank") / "resample_bank_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["resample_bank_host.h"]          # the host header only
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


# ------------------------------------------------------------------------------------------------ resample_bank_host.h
def test_host_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "resample_bank_host.h")).read()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', txt) == ["resample_host.h"]
    assert "hip" not in re.sub(r"//.*", "", txt).lower().replace("__hipcc__", "")


def test_rows_follow_their_single_pair_twins_under_the_sanitizers(check, tmp_path):
    """Random per-row schedules of blocks, holds, flushes, resets and re-assignments over six pairs, one of them walked in chunks
    (chunk < ld), some rounds starting near 2^40: counts, positions, descriptor fields and the kernel's tile arithmetic against a
    single-pair stream computed from resample_host.h alone.  The program's own checks, run plain and under
    -fsanitize=address,undefined."""
    assert check("self") == ["ok"]
    exe = str(tmp_path / "resample_bank_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    out = subprocess.run([exe, "self"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def reduced(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    up, down = rate_out // g, rate_in // g
    return up, down, 10 * max(up, down)


def ready(N, up, down, half):
    if N < 1:
        return 0
    a = N * up - half - 1
    return min(0 if a < 0 else a // down + 1, -(-N * up // down))


def test_descriptor_fields_near_2_to_the_40(check):
    """Positions near 2^40 (J * down near 2^50), against Python's integers: every field of the descriptor is a difference from the row's
    carry origin or a residue below `up`, none needs more than 32 bits, and the next position is the single-pair rule."""
    rnd = random.Random(11)
    for pair in [(48000, 44100), (44100, 48000), (16000, 44100), (44100, 8000), (192000, 44100), (1000, 1), (1, 1000), (44100, 44100)]:
        up, down, half = reduced(*pair)
        kh = half // up
        for case in range(8):
            N = (1 << 40) + rnd.randrange(-70000, 70000) if case else 0
            J = ready(N, up, down, half)
            cur, k = rnd.randrange(2), rnd.randrange(16)
            flush = case % 4 == 3
            n_in = 0 if flush else rnd.choice([1, 7, 1024, 1115, 250000])
            got = [int(v) for v in check("desc", pair[0], pair[1], N, J, cur, k, n_in, int(flush))[0].split()]
            origin = max(0, J * down // up - kh)
            N1 = N + n_in
            J1 = -(-N1 * up // down) if flush else ready(N1, up, down, half)
            runs = int(J1 > J or not flush)
            if not runs:
                assert got[:12] == [0, 0, 0, 0, 0, 0, 0, 0, k, cur, 0, 0]
            else:
                assert got[:12] == [0, n_in, J1 - J, max(0, J1 * down // up - kh) - origin, N - origin, J * down // up - origin,
                                    J * down % up, J % up, k, cur, 1, int(not flush)], (pair, case)
                assert 0 <= got[4] <= 2 * half // up + down // up + 2 and got[4] < 1 << 16          # the carry, and its 16 bits
                assert 0 <= got[5] <= kh < 1 << 16 and got[6] < 1 << 10 and got[7] < 1 << 10
                assert all(0 <= v < 1 << 31 for v in got[1:4])
            assert got[12:] == ([0, 0, cur] if flush else [N1, J1, cur ^ 1])


def test_group_of_descriptors_fits_the_argument_space(check):
    """The header states 4096 bytes of kernel-argument space, 256 of them the compiler's own arguments and 256 kept for the kernel's
    other arguments: a group is as many 20-byte descriptors as the rest holds, and the launch structure beside it is within its share."""
    row, group, size, space, implicit, other = [int(v) for v in check("group")[0].split()]
    assert (row, space, implicit, other) == (20, 4096, 256, 256)
    assert group == (space - implicit - other) // row == 179 and size == group * row
    assert size + implicit + other <= space < size + row + implicit + other
    assert group >= 64                                             # a 64-row pool is one launch
    k = open(os.path.join(CSRC, "kernels.h")).read()
    assert re.search(r"static_assert\(sizeof\(BankLaunch\) <= BANK_ARG_OTHER", k)
    assert "179" in open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    bank = "bsrnn_resampler_bank*"
    want = {
        "bsrnn_resampler_bank_create": ("int", ["bsrnn_ctx*", "int32_t", "constint32_t*", "constint32_t*", "int32_t", "bsrnn_resampler_bank**"]),
        "bsrnn_resampler_bank_destroy": ("void", [bank]),
        "bsrnn_resampler_bank_assign": ("int", [bank, "constint32_t*", "int32_t", "int32_t"]),
        "bsrnn_resampler_bank_pair_of": ("int", ["const" + bank, "int32_t"]),
        "bsrnn_resampler_bank_ready": ("int64_t", ["const" + bank, "int32_t", "int64_t"]),
        "bsrnn_resampler_bank_process": ("int", [bank, "constfloat*", "int64_t", "constint64_t*", "float*", "int64_t", "int64_t*", "void*"]),
        "bsrnn_resampler_bank_flush_rows": ("int", [bank, "constint32_t*", "int32_t", "float*", "int64_t", "int64_t*", "void*"]),
        "bsrnn_resampler_bank_reset_rows": ("int", [bank, "constint32_t*", "int32_t"]),
    }
    for name, (ret, types) in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, body, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, name
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body) and re.search(r"#define\s+BSRNN_BANK_PAIRS_MAX\s+16\b", body)


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_resampler_bank_process.argtypes == [vp, vp, i64, ctypes.POINTER(i64), vp, i64, ctypes.POINTER(i64), vp]
    assert native.lib.bsrnn_resampler_bank_ready.restype == i64 and native.lib.bsrnn_resampler_bank_ready.argtypes == [vp, i32, i64]
    assert native.BANK_PAIRS_MAX == 16 and native.lib.bsrnn_abi_version() == 2


def test_argument_errors_without_a_device(native, host_ctx):
    """What bsrnn_resampler_bank_create refuses, in front of the BSRNN_ESTATE of a host-only context, and the null object everywhere.
    (Rows, pairs, counts and strides of a LIVE bank: tests/test_gpu_resample_bank.py - a bank exists only on a device.)"""
    lib = native.lib

    def err():
        return lib.bsrnn_last_error().decode()

    def rates(*v):
        return (ctypes.c_int32 * len(v))(*v)
    bank = ctypes.c_void_p()
    make = lib.bsrnn_resampler_bank_create
    good_in, good_out = rates(48000, 16000), rates(44100, 44100)
    assert make(None, 4, good_in, good_out, 2, ctypes.byref(bank)) == EARG
    assert make(host_ctx, 0, good_in, good_out, 2, ctypes.byref(bank)) == EARG
    assert "C = 0" in err(), err()
    assert make(host_ctx, 4, good_in, good_out, 2, None) == EARG
    assert make(host_ctx, 4, good_in, good_out, 0, ctypes.byref(bank)) == EARG
    assert "n_pairs = 0" in err() and "[1, 16]" in err(), err()
    assert make(host_ctx, 4, rates(*[48000] * 17), rates(*[44100] * 17), 17, ctypes.byref(bank)) == EARG
    assert "n_pairs = 17" in err(), err()
    assert make(host_ctx, 4, None, good_out, 2, ctypes.byref(bank)) == EARG
    assert make(host_ctx, 4, rates(48000, 0), good_out, 2, ctypes.byref(bank)) == EARG
    assert "rate_in = 0" in err(), err()
    assert make(host_ctx, 4, good_in, rates(44100, 48001), 2, ctypes.byref(bank)) == EARG          # 16000 -> 48001 does not reduce
    assert "48001 / 16000" in err() and "1024" in err(), err()
    assert make(host_ctx, 4, good_in, good_out, 2, ctypes.byref(bank)) == ESTATE
    assert "host-only" in err(), err()
    assert make(host_ctx, 4, rates(*[48000] * 16), rates(*[44100] * 16), 16, ctypes.byref(bank)) == ESTATE
    assert not bank.value
    # null objects
    a = np.zeros((2, 10), np.float32)
    pa = a.ctypes.data_as(ctypes.c_void_p)
    n_in, n_out, rows = (ctypes.c_int64 * 2)(5, 5), (ctypes.c_int64 * 2)(-5, -5), rates(0, 1)
    assert lib.bsrnn_resampler_bank_process(None, pa, 10, n_in, pa, 10, n_out, None) == EARG
    assert "null" in err(), err()
    assert lib.bsrnn_resampler_bank_flush_rows(None, rows, 2, pa, 10, n_out, None) == EARG
    assert lib.bsrnn_resampler_bank_assign(None, rows, 2, 0) == EARG
    assert lib.bsrnn_resampler_bank_reset_rows(None, rows, 2) == EARG
    assert lib.bsrnn_resampler_bank_ready(None, 0, 10) == -1 and lib.bsrnn_resampler_bank_pair_of(None, 0) == -1
    assert list(n_out) == [-5, -5]
    lib.bsrnn_resampler_bank_destroy(None)


# ------------------------------------------------------------------------------------------------ Python layer
def test_python_layer_signatures_and_refusals_before_any_device_work(native):
    import torch
    from speechseparation_amd.bsrnn import BSRNN, ResamplerBank, StreamPool
    assert list(inspect.signature(ResamplerBank.__init__).parameters) == ["self", "model", "channels", "pairs"]
    for name, args in (("assign", ["self", "rows", "pair"]), ("ready", ["self", "row", "n"]), ("process", ["self", "wave", "counts"]),
                       ("flush_rows", ["self", "rows"]), ("reset_rows", ["self", "rows"])):
        assert list(inspect.signature(getattr(ResamplerBank, name)).parameters) == args
    sig = inspect.signature(StreamPool)                  # the call of the class: __init__'s parameters (test_stream_rows_host.py holds those)
    assert list(sig.parameters) == ["model", "slots", "rows_per_session", "device", "rates"] and sig.parameters["rates"].default is None
    assert sig.parameters["rows_per_session"].default == 1 and sig.parameters["device"].default is None
    assert StreamPool(BSRNN(), 3, 2, None, (48000,)).rates == (48000,) and StreamPool(BSRNN(), 3, rates=[16000]).rates == (16000,)
    assert StreamPool(BSRNN(), 3).rates is None and StreamPool(BSRNN(), 3, rows_per_session=2, device="cuda:0").rows == 2
    sig = inspect.signature(StreamPool.open)
    assert list(sig.parameters) == ["self", "sample_rate"] and sig.parameters["sample_rate"].default is None
    assert callable(StreamPool.drain) and "resample_len" in StreamPool.drain.__doc__ and "44.1" in StreamPool.pending.__doc__
    m = BSRNN()
    for bad in (lambda: ResamplerBank(m, 2, []),                                        # no pair
                lambda: ResamplerBank(m, 2, [(48000, 44100)] * 17),                     # more than 16
                lambda: ResamplerBank(m, 2, [(48000, 44100), (0, 44100)]),
                lambda: ResamplerBank(m, 2, [(44100, 48001)]),                          # reduces beyond 1024
                lambda: ResamplerBank(m, 0, [(48000, 44100)]),
                lambda: ResamplerBank(m, 2, 48000),
                lambda: StreamPool(m, 4, 2, rates=()),
                lambda: StreamPool(m, 4, 2, rates=(48000,) * 17),
                lambda: StreamPool(m, 4, 2, rates=(16000, 0)),
                lambda: StreamPool(m, 4, 2, rates=(16000, 48001)),                      # 48001 / 44100 does not reduce
                lambda: StreamPool(m, 4, 2, rates=(16000, 48000.0)),
                lambda: StreamPool(m, 4, 2, rates=48000)):
        with pytest.raises(ValueError):
            bad()
    pool = StreamPool(m, 2, 2, rates=(16000, 48000))
    with pytest.raises(ValueError, match="8000"):
        pool.open(sample_rate=8000)                                                     # not one of the pool's
    plain = StreamPool(m, 2, 2)
    with pytest.raises(ValueError, match="48000"):
        plain.open(sample_rate=48000)                                                   # a pool without rates has none to offer
    assert plain.sessions() == [] and pool.sessions() == []                             # a refused open takes no slot
    a, b, c = pool.open(sample_rate=48000), pool.open(), plain.open(sample_rate=44100)
    assert pool.rate_of(a) == 48000 and pool.rate_of(b) == 44100 and plain.rate_of(c) == 44100
    # step() refuses a session with a rate by name, before it looks for a device; export() likewise
    with pytest.raises(ValueError, match=r"feed\(\)"):
        pool.step({a: torch.zeros((2, 1024)), b: torch.zeros((2, 1024))})
    with pytest.raises(ValueError, match="sample rate"):
        pool.export(a)
    with pytest.raises(ValueError):
        pool.feed({a: torch.zeros((3, 100))})                                           # the shape check of feed() comes first as before
    with pytest.raises(ValueError):
        pool.drain(a, mix="wet")
    pool.close(a)
    with pytest.raises(ValueError):
        pool.open(sample_rate=96000)
    assert pool.open(sample_rate=16000) == 2 and pool.rate_of(2) == 16000
    assert m._ctx is None and pool._st is None and pool._bank_in is None and plain._st is None
