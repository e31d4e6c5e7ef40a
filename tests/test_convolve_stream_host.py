"""CPU-side tests of the streaming FIR convolution (bsrnn_fir_stream_*): the arithmetic of csrc/convolve_stream_host.h - what a row has
been handed, the blocks of a call, the flush plan, the ring - against a brute-force restatement in Python (through
tests/cpp/convolve_stream_check.cpp, built with -Wall -Werror and a second time with the address and undefined-behaviour sanitizers); the
float32 model of the stream against convolve_reference.ref32 (bit for bit) and, under the causal alignment, against the float64
definition; declarations, exports, bindings and argument refusals on a host-only context.  No compute here;
tests/test_gpu_convolve_stream.py holds the kernel."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import convolve_reference as cr
import convolve_stream_reference as sr
from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "convolve_stream_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
B = 1024
KS = [1, 2, 3, 1023, 1024, 1025, 2048, 2049, 9300, 262144]
NS = [1, 1023, 1024, 1025, 2047, 2500, 9221]
NEW = ["bsrnn_fir_stream_create", "bsrnn_fir_stream_destroy", "bsrnn_fir_stream_assign", "bsrnn_fir_stream_filter_of", "bsrnn_fir_stream_ready",
       "bsrnn_fir_stream_process", "bsrnn_fir_stream_flush_rows", "bsrnn_fir_stream_reset_rows"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output lines."""
    exe = str(tmp_path_factory.mktemp("convolve_stream") / "convolve_stream_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["convolve_stream_host.h"]          # the new header only
    assert re.findall(r'#include\s+"([^"]+)"', open(os.path.join(CSRC, "convolve_stream_host.h")).read()) == ["convolve_host.h"]
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


# ------------------------------------------------------------------------------------------------ convolve_stream_host.h
def test_self_checks_under_the_sanitizers(check, tmp_path):
    assert check("self") == ["ok"]
    exe = str(tmp_path / "convolve_stream_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    for args in (["self"], ["cut", "262144", "0", "1000", "0", "8221"], ["rows", "9300", "1", "1025", "3000"]):
        out = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0 and out.stdout.strip(), out.stdout + out.stderr
    assert check("limits") == ["0 1 %d %d 2048" % (1 << 30, (2 ** 63 - 1) // 4)]


@pytest.mark.parametrize("align", [sr.SAME, sr.CAUSAL])
@pytest.mark.parametrize("k", KS)
def test_counts_blocks_and_flush_against_brute_force(check, k, align):
    """From the definition alone: the blocks a call walks are the frames it completes; what it hands out are the output samples of those
    blocks (y[m] lies in block (m + shift) // B); ready is that count; after the flush the counts sum to N; under the SAME alignment the
    flush plan is conv_plan(N, k)'s."""
    shift = sr.shift_of(k, align)
    for n in NS:
        for name, cuts in sr.cuttings(n, 1000 * k + n).items():
            lines = [[int(v) for v in ln.split()] for ln in check("cut", k, align, *cuts)]
            calls, (u1, f1, n_out) = sr.plan(k, align, cuts)
            assert len(lines) == len(cuts) + 1
            at = handed = 0
            for (first, count, ready, before), want, c in zip(lines, calls, cuts):
                assert (first, count, ready) == want, (k, n, name, at)
                assert before == handed == sr.emitted(at, shift)
                at += c
                handed += ready
            got_shift, u0, got_u1, got_f1, first, count, got_out, m0, m1 = lines[-1]
            assert (got_shift, u0, got_u1, got_f1, got_out) == (shift, shift // B, u1, f1, n_out), (k, n, name)
            assert handed + got_out == n                                   # the counts sum to N after the flush
            assert first == n // B and count == max(0, u1 - first + 1)
            assert (m0, m1) == (max(0, u1 * B - shift), n)                 # the last store ends the row
            if align == sr.SAME:
                assert cr.plan(n, k)[1:4] == (shift, u0, u1) and cr.plan(n, k)[5] == f1
            # the kernel's descriptors say the same
            rows = [[int(v) for v in ln.split()] for ln in check("rows", k, align, *cuts)]
            at = 0
            for (N0, E0, sh, n_end, ub, ue, r_u0, r_f1, n_in, P, keep), (first, count, ready), c in zip(rows, calls, cuts):
                if c == 0:
                    assert (ub, ue, n_in) == (0, 0, 0)                     # held
                else:
                    assert (N0, E0, sh, ub, ue - ub, r_u0, n_in, P, keep) == (at, sr.emitted(at, shift), shift, first, count, shift // B, c, -(-k // B), 1)
                    assert n_end > 1 << 60 and r_f1 > 1 << 60
                at += c
            N0, E0, sh, n_end, ub, ue, r_u0, r_f1, n_in, P, keep = rows[-1]
            if n_out:
                assert (N0, E0, sh, n_end, ub, ue, r_u0, r_f1, n_in, P, keep) == (n, n - n_out, shift, n, n // B, u1 + 1, shift // B, f1, 0, -(-k // B), 0)
            else:
                assert ub == ue and n_in == 0


def test_no_ring_slot_is_overwritten_before_its_last_reader():
    """Block u reads frames u - p, p <= min(P - 1, u), from slots (u - p) mod P; frame v is written into slot v mod P when block v is
    walked.  Walking blocks in order, the slot of every frame a block reads still holds that frame - and with P - 1 slots it would not."""
    for P in (1, 2, 3, 44, 256):
        for slots, ok in ((P, True), (P - 1, False)):
            if slots < 1:
                continue
            held, clean = {}, True
            for u in range(3 * P + 2):
                held[u % slots] = u
                clean &= all(held.get((u - p) % slots) == u - p for p in range(min(P - 1, u) + 1))
            assert clean == ok, (P, slots)


# ------------------------------------------------------------------------------------------------ the float32 model
@pytest.mark.parametrize("name", [c[0] for c in cr.CASES])
def test_model_equals_ref32_for_every_cutting(name):
    x, h, r32, r64 = cr.case(name)
    for cut, cuts in sr.cuttings(x.shape[0], 300 + ord(name)).items():
        got = sr.StreamModel(h).run(x, cuts)
        assert got.dtype == np.float32 and np.array_equal(got, r32), (name, cut)


def test_model_continues_after_a_flush_as_a_fresh_stream():
    x, h, r32, r64 = cr.case("g")
    m = sr.StreamModel(h)
    m.run(cr.case("f")[0], [1500, 1500])                                   # leaves a ring, a tail and (had there been no flush) a FIFO behind
    assert np.array_equal(m.run(x, [700, 4300]), r32)


@pytest.mark.parametrize("name", [c[0] for c in cr.CASES])
def test_causal_model_meets_the_criterion(name):
    x, h, _, _ = cr.case(name)
    r32, r64 = sr.causal_refs(x, h)
    for cut, cuts in sr.cuttings(x.shape[0], 400 + ord(name)).items():
        got = sr.StreamModel(h, sr.CAUSAL).run(x, cuts)
        assert got.shape == r64.shape
        cr.hold_row("case %s, causal, %s" % (name, cut), got, r32, r64)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {
        "bsrnn_fir_stream_create": ("int", ["bsrnn_fir_bank*", "int32_t", "int32_t", "int32_t", "bsrnn_fir_stream**"]),
        "bsrnn_fir_stream_destroy": ("void", ["bsrnn_fir_stream*"]),
        "bsrnn_fir_stream_assign": ("int", ["bsrnn_fir_stream*", "constint32_t*", "int32_t", "int32_t"]),
        "bsrnn_fir_stream_filter_of": ("int32_t", ["constbsrnn_fir_stream*", "int32_t"]),
        "bsrnn_fir_stream_ready": ("int64_t", ["constbsrnn_fir_stream*", "int32_t", "int64_t"]),
        "bsrnn_fir_stream_process": ("int", ["bsrnn_fir_stream*", "constfloat*", "int64_t", "constint64_t*", "float*", "int64_t", "int64_t*", "void*"]),
        "bsrnn_fir_stream_flush_rows": ("int", ["bsrnn_fir_stream*", "constint32_t*", "int32_t", "float*", "int64_t", "int64_t*", "void*"]),
        "bsrnn_fir_stream_reset_rows": ("int", ["bsrnn_fir_stream*", "constint32_t*", "int32_t"]),
    }
    for name, (ret, types) in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, body, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, (name, got)
    assert re.search(r"#define\s+BSRNN_FIR_SAME\s+0\b", body) and re.search(r"#define\s+BSRNN_FIR_CAUSAL\s+1\b", body)
    assert re.search(r"typedef\s+struct\s+bsrnn_fir_stream\s+bsrnn_fir_stream\s*;", body)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body)


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    pi32, pi64 = ctypes.POINTER(i32), ctypes.POINTER(i64)
    lib = native.lib
    assert lib.bsrnn_fir_stream_create.argtypes == [vp, i32, i32, i32, ctypes.POINTER(vp)]
    assert lib.bsrnn_fir_stream_assign.argtypes == [vp, pi32, i32, i32]
    assert lib.bsrnn_fir_stream_process.argtypes == [vp, vp, i64, pi64, vp, i64, pi64, vp]
    assert lib.bsrnn_fir_stream_flush_rows.argtypes == [vp, pi32, i32, vp, i64, pi64, vp]
    assert lib.bsrnn_fir_stream_reset_rows.argtypes == [vp, pi32, i32]
    assert lib.bsrnn_fir_stream_filter_of.argtypes == [vp, i32] and lib.bsrnn_fir_stream_filter_of.restype == i32
    assert lib.bsrnn_fir_stream_ready.argtypes == [vp, i32, i64] and lib.bsrnn_fir_stream_ready.restype == i64
    assert lib.bsrnn_fir_stream_destroy.restype is None
    assert lib.bsrnn_abi_version() == 2


def test_argument_errors_without_a_device(native, host_ctx):
    """Every refusal of the interface on a host-only context, with its sentence, followed by a valid call; BSRNN_ESTATE comes after the
    checks.  The counts a host-only stream answers are the header's."""
    lib = native.lib

    def err():
        return lib.bsrnn_last_error().decode()
    i64s, i32s = (lambda *v: (ctypes.c_int64 * len(v))(*v)), (lambda *v: (ctypes.c_int32 * len(v))(*v))
    f0, f1 = np.ones(3, np.float32), np.ones(1500, np.float32)
    bank = ctypes.c_void_p()
    assert lib.bsrnn_fir_bank_create(host_ctx, 2, (ctypes.c_void_p * 2)(f0.ctypes.data, f1.ctypes.data), i32s(3, 1500), ctypes.byref(bank)) == 0
    st = ctypes.c_void_p()
    make = lib.bsrnn_fir_stream_create
    assert make(None, 3, 1500, 0, ctypes.byref(st)) == EARG and "null FIR bank" in err(), err()
    assert make(bank, 3, 1500, 0, None) == EARG
    for bad in (0, -1):
        assert make(bank, bad, 1500, 0, ctypes.byref(st)) == EARG and "C = %d" % bad in err(), err()
    for bad in (0, -5, 262145):
        assert make(bank, 3, bad, 0, ctypes.byref(st)) == EARG and "max_taps = %d" % bad in err() and "262144" in err(), err()
    for bad in (-1, 2):
        assert make(bank, 3, 1500, bad, ctypes.byref(st)) == EARG and "align = %d" % bad in err(), err()
    assert not st.value
    assert make(bank, 3, 1000, 0, ctypes.byref(st)) == 0 and st.value      # a valid call: a host-only stream answers counts and refusals
    # all rows start on bypass
    assert [lib.bsrnn_fir_stream_filter_of(st, r) for r in (-1, 0, 1, 2, 3)] == [-2, -1, -1, -1, -2] and lib.bsrnn_fir_stream_filter_of(None, 0) == -2
    assert lib.bsrnn_fir_stream_ready(st, 1, 777) == 777
    assign = lib.bsrnn_fir_stream_assign
    assert assign(None, i32s(0), 1, 0) == EARG and "null FIR stream" in err()
    for bad in (-2, 2):
        assert assign(st, i32s(0), 1, bad) == EARG and "filter %d" % bad in err() and "[-1, 2)" in err(), err()
    assert assign(st, i32s(0), 1, 1) == EARG and "1500 taps" in err() and "max_taps = 1000" in err(), err()
    assert assign(st, None, 1, 0) == EARG and "n_rows = 1" in err(), err()
    assert assign(st, i32s(0), -1, 0) == EARG and "n_rows = -1" in err(), err()
    for bad in (-1, 3):
        assert assign(st, i32s(0, bad), 2, 0) == EARG and "row %d" % bad in err() and "[0, 3)" in err(), err()
    assert assign(st, i32s(1, 1), 2, 0) == EARG and "row 1 is listed twice" in err(), err()
    assert [lib.bsrnn_fir_stream_filter_of(st, r) for r in range(3)] == [-1, -1, -1]          # the object is untouched
    assert assign(st, i32s(0, 2), 2, 0) == 0 and assign(st, None, 0, 0) == 0
    assert [lib.bsrnn_fir_stream_filter_of(st, r) for r in range(3)] == [0, -1, 0]
    # ready: k = 3, shift 1: the first hop hands out 1023
    ready = lib.bsrnn_fir_stream_ready
    assert [ready(st, 0, n) for n in (0, 1023, 1024, 2048, 1 << 30)] == [0, 0, 1023, 2047, (1 << 30) - 1]
    assert ready(None, 0, 5) == -1 and ready(st, 3, 5) == -1 and ready(st, -1, 5) == -1 and ready(st, 0, -1) == -1 and ready(st, 0, (1 << 30) + 1) == -1
    reset = lib.bsrnn_fir_stream_reset_rows
    assert reset(None, i32s(0), 1) == EARG and "null FIR stream" in err()
    assert reset(st, i32s(3), 1) == EARG and "row 3" in err() and reset(st, i32s(0, 0), 2) == EARG and "listed twice" in err()
    assert reset(st, None, 2) == EARG and "n_rows = 2" in err()
    assert reset(st, i32s(0, 1), 2) == 0
    # process
    a, b = np.zeros((3, 2000), np.float32), np.zeros((3, 2000), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    n_out = i64s(-7, -7, -7)
    proc = lib.bsrnn_fir_stream_process
    good = (st, pa, 2000, i64s(1500, 100, 0), pb, 2000, n_out, None)
    assert proc(None, *good[1:]) == EARG and "null FIR stream" in err()
    assert proc(st, pa, 2000, None, pb, 2000, n_out, None) == EARG and "sample counts" in err(), err()
    assert proc(st, pa, 2000, i64s(1500, 100, 0), pb, 2000, None, None) == EARG and "nowhere to report" in err(), err()
    assert proc(st, None, 2000, i64s(1500, 100, 0), pb, 2000, n_out, None) == EARG and "input block" in err(), err()
    assert proc(st, pa, 2000, i64s(1500, 100, 0), None, 2000, n_out, None) == EARG and "output block" in err(), err()
    for bad in (-1, (1 << 30) + 1):
        assert proc(st, pa, 1 << 31, i64s(1500, bad, 0), pb, 1 << 31, n_out, None) == EARG and "n_in_host[1] = %d" % bad in err(), err()
    assert proc(st, pa, 1499, i64s(1500, 100, 0), pb, 2000, n_out, None) == EARG and "in_stride = 1499" in err() and "1500" in err(), err()
    # row 0 (k = 3) is handed 1023, row 1 (bypass) its 100: the stride must hold 1023
    assert proc(st, pa, 2000, i64s(1500, 100, 0), pb, 1022, n_out, None) == EARG and "out_stride = 1022" in err() and "1023" in err(), err()
    assert proc(st, pa, 2000, i64s(1500, 100, 0), pa, 2000, n_out, None) == EARG and "overlap" in err(), err()
    last = ctypes.c_void_p(pa.value + 4 * (2 * 2000 + 1499))              # the last float the rows of the input span
    assert proc(st, pa, 2000, i64s(1500, 100, 0), last, 2000, n_out, None) == EARG and "overlap" in err(), err()
    assert list(n_out) == [-7, -7, -7]                                     # nothing was reported by a refused call
    assert proc(*good) == ESTATE and "host-only" in err(), err()           # valid arguments: a host-only context cannot compute
    assert [ready(st, 0, n) for n in (1023, 1024)] == [0, 1023]            # ... and the object is untouched
    # flush
    flush = lib.bsrnn_fir_stream_flush_rows
    assert flush(None, i32s(0), 1, pb, 2000, n_out, None) == EARG and "null FIR stream" in err()
    assert flush(st, i32s(0), 1, pb, 2000, None, None) == EARG and "nowhere to report" in err()
    assert flush(st, i32s(5), 1, pb, 2000, n_out, None) == EARG and "row 5" in err()
    assert flush(st, i32s(2, 2), 2, pb, 2000, n_out, None) == EARG and "listed twice" in err()
    assert flush(st, None, 1, pb, 2000, n_out, None) == EARG and "n_rows = 1" in err()
    assert flush(st, i32s(0), 1, None, 0, n_out, None) == ESTATE           # rows that took nothing are owed nothing: no block is needed
    assert not a.any() and not b.any()
    # the bank may go first: the stream keeps it alive
    lib.bsrnn_fir_bank_destroy(bank)
    assert ready(st, 0, 1024) == 1023 and assign(st, i32s(1), 1, 1) == EARG and "1500 taps" in err()
    lib.bsrnn_fir_stream_destroy(st)
    lib.bsrnn_fir_stream_destroy(None)


def test_python_layer_signatures():
    import inspect
    from speechseparation_amd import augment
    sig = inspect.signature(augment.FirStream.__init__)
    assert list(sig.parameters) == ["self", "bank", "rows", "max_taps", "causal"]
    assert sig.parameters["max_taps"].default is None and sig.parameters["causal"].default is False
    assert list(inspect.signature(augment.FirStream.assign).parameters) == ["self", "rows", "filter"]
    assert list(inspect.signature(augment.FirStream.filter_of).parameters) == ["self", "row"]
    assert list(inspect.signature(augment.FirStream.ready).parameters) == ["self", "row", "n"]
    sig = inspect.signature(augment.FirStream.process)
    assert list(sig.parameters) == ["self", "wave", "counts", "out"] and sig.parameters["counts"].default is None and sig.parameters["out"].default is None
    sig = inspect.signature(augment.FirStream.flush)
    assert list(sig.parameters)[:2] == ["self", "rows"] and sig.parameters["rows"].default is None
    sig = inspect.signature(augment.FirStream.reset)
    assert list(sig.parameters) == ["self", "rows"] and sig.parameters["rows"].default is None
