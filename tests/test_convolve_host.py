"""CPU-side tests of the long FIR convolution (bsrnn_fir_bank_*, bsrnn_convolve_ragged): the plan of csrc/convolve_host.h - blocks, store
ranges, partition spans, row groups - against a brute-force restatement in Python (through tests/cpp/convolve_plan_check.cpp, built with
-Wall -Werror and a second time with the address and undefined-behaviour sanitizers); the float32 reference of the GPU tests against the
float64 definition, and the criterion against a result with one wrong block; declarations, exports, bindings and argument refusals on a
host-only context.  No compute here; tests/test_gpu_convolve.py holds the kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import convolve_reference as cr
from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "convolve_plan_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
B = 1024
KS = [1, 2, 3, 1023, 1024, 1025, 2048, 2049, 9300, 262144]
NS = [1, 2, 1023, 1024, 1025, 2047, 2500, 9221]
NEW = ["bsrnn_fir_bank_create", "bsrnn_fir_bank_destroy", "bsrnn_fir_bank_count", "bsrnn_fir_bank_taps", "bsrnn_convolve_ragged"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output lines."""
    exe = str(tmp_path_factory.mktemp("convolve") / "convolve_plan_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["convolve_host.h"]          # the host header only
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


# ------------------------------------------------------------------------------------------------ convolve_host.h
def test_self_checks_under_the_sanitizers(check, tmp_path):
    assert check("self") == ["ok"]
    exe = str(tmp_path / "convolve_plan_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    for args in (["self"], ["ranges", "262144", "9221"], ["groups", "10", "4:3", "7:7", "0:0", "12:11"]):
        out = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0 and out.stdout.strip(), out.stdout + out.stderr
    assert check("limits") == ["1024 2050 262144 %d 65536 32768 16" % (1 << 40)]


@pytest.mark.parametrize("k", KS)
def test_ranges_against_brute_force(check, k):
    """From the definition alone: y[m] = (x * g)[m + shift] lies in block (m + shift) // B; (x * g)[i] = sum_j x[i - j] g[j] reads partition
    j // B.  Every y[m] is stored exactly once, nothing is stored outside [0, n), no block is computed that stores nothing, every partition
    a block needs is in its span, and every partition of a span has its frame among the transformed ones."""
    P, shift = -(-k // B), k // 2
    for n in NS:
        lines = check("ranges", k, n)
        got_P, got_shift, u0, u1, f0, f1 = (int(v) for v in lines[0].split())
        assert (got_P, got_shift) == (P, shift)
        blocks = [[int(v) for v in ln.split()] for ln in lines[1:]]
        assert [b[0] for b in blocks] == list(range(u0, u1 + 1))
        stored = np.zeros(n, np.int64)
        m = np.arange(n)
        owner = (m + shift) // B                                         # the block every output sample comes from
        assert u0 == owner.min() and u1 == owner.max()
        frames_read = set()
        for u, m0, m1, p_lo, p_hi in blocks:
            assert 0 <= m0 < m1 <= n, (k, n, u)                          # stores something, inside the row
            stored[m0:m1] += 1
            assert (owner[m0:m1] == u).all() and m0 + shift >= u * B and m1 - 1 + shift < (u + 1) * B
            # the partitions the block's samples i in [u B, (u + 1) B) need: taps j in [p B, min((p + 1) B, k)), x[i - j] inside [0, n)
            need = [p for p in range(P) if (u + 1) * B - 1 - p * B >= 0 and u * B - (min((p + 1) * B, k) - 1) <= n - 1]
            assert need and set(need) <= set(range(p_lo, p_hi + 1)), (k, n, u, need, p_lo, p_hi)
            assert 0 <= p_lo <= p_hi <= P - 1
            for p in range(p_lo, p_hi + 1):
                assert f0 <= u - p <= f1
                frames_read.add(u - p)
        assert (stored == 1).all(), (k, n)
        assert frames_read == set(range(f0, f1 + 1)), (k, n)             # no frame is transformed that no block reads
        # the Python restatement the float32 reference uses is the same plan
        assert cr.plan(n, k) == (P, shift, u0, u1, f0, f1)


def test_row_groups_around_the_budget(check):
    budget = 65536
    rows = lambda nx, nb, R: ["%d:%d" % (nx, nb)] * R                     # noqa: E731

    def groups(*args):
        return [tuple(int(v) for v in ln.split()) for ln in check("groups", *args)]
    assert groups(budget, *rows(978, 977, 67)) == [(0, 67, 67 * 978, 67 * 977)]                      # 65526 frames: one group
    assert groups(budget, *rows(978, 977, 68)) == [(0, 67, 67 * 978, 67 * 977), (67, 1, 978, 977)]   # 66504: the 68th row starts another
    assert groups(budget, *rows(978, 977, 70)) == [(0, 67, 67 * 978, 67 * 977), (67, 3, 3 * 978, 3 * 977)]
    assert groups(budget, "65536:65536") == [(0, 1, 65536, 65536)]
    assert groups(budget, "65536:65535", "1:1") == [(0, 1, 65536, 65535), (1, 1, 1, 1)]
    assert groups(budget, "65535:65536", "0:0", "1:1") == [(0, 2, 65535, 65536), (2, 1, 1, 1)]       # a copied row costs nothing
    assert groups(budget, "70000:70000", "5:5") == [(0, 1, 70000, 70000), (1, 1, 5, 5)]              # a row beyond the budget: alone
    assert groups(budget, "5:5", "70000:70000", "5:5") == [(0, 1, 5, 5), (1, 1, 70000, 70000), (2, 1, 5, 5)]
    assert groups(10, "4:3", "7:7", "0:0", "12:11") == [(0, 1, 4, 3), (1, 2, 7, 7), (3, 1, 12, 11)]


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", [c[0] for c in cr.CASES])
def test_ref32_meets_the_criterion(name):
    x, h, r32, r64 = cr.case(name)
    m = cr.hold_row("case %s: ref32 against ref64" % name, r32, r32, r64)
    # and float32 it is: the algorithm's error is a few 1e-7 of the output's peak, not more
    assert m["e32"] <= 2e-6 * m["peak"], m


@pytest.mark.parametrize("name", [c[0] for c in cr.CASES])
def test_criterion_rejects_one_wrong_block(name):
    """Partition P - 1 dropped from one block: rejected, in the max-abs form or in the per-block form.  (Cases h and j, a filter longer
    than the row: no block reads partition P - 1 - it meets only frames past the row's end - so the last partition that is read.)"""
    x, h, r32, r64 = cr.case(name)
    n, k = x.shape[0], h.shape[0]
    u, p = cr.block_with_last_partition(n, k)
    assert p == -(-k // B) - 1 or k > n
    wrong = cr.ref32(x, h, drop=(u, p))
    assert not np.array_equal(wrong, r32)
    with pytest.raises(AssertionError):
        cr.hold_row("case %s: block %d without partition %d" % (name, u, p), wrong, r32, r64)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {
        "bsrnn_fir_bank_create": ("int", ["bsrnn_ctx*", "int32_t", "constfloat*const*", "constint32_t*", "bsrnn_fir_bank**"]),
        "bsrnn_fir_bank_destroy": ("void", ["bsrnn_fir_bank*"]),
        "bsrnn_fir_bank_count": ("int32_t", ["constbsrnn_fir_bank*"]),
        "bsrnn_fir_bank_taps": ("int32_t", ["constbsrnn_fir_bank*", "int32_t"]),
        "bsrnn_convolve_ragged": ("int", ["bsrnn_fir_bank*", "constfloat*", "int64_t", "constint64_t*", "constint32_t*", "float*", "int64_t",
                                          "int32_t", "void*"]),
    }
    for name, (ret, types) in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, body, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, (name, got)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body)
    assert "m_dataset.py:92-114" in txt and "padding='same'" in txt


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_convolve_ragged.argtypes == [vp, vp, i64, ctypes.POINTER(i64), ctypes.POINTER(i32), vp, i64, i32, vp]
    assert native.lib.bsrnn_fir_bank_count.restype == i32 and native.lib.bsrnn_fir_bank_taps.restype == i32
    assert native.lib.bsrnn_abi_version() == 2


def make_bank(lib, ctx, filters):
    n = len(filters)
    ptrs = (ctypes.c_void_p * n)(*[f.ctypes.data for f in filters])
    counts = (ctypes.c_int32 * n)(*[f.shape[0] for f in filters])
    bank = ctypes.c_void_p()
    return lib.bsrnn_fir_bank_create(ctx, n, ptrs, counts, ctypes.byref(bank)), bank


def test_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib

    def err():
        return lib.bsrnn_last_error().decode()
    f0, f1 = np.ones(3, np.float32), np.ones(1500, np.float32)
    ptrs = (ctypes.c_void_p * 2)(f0.ctypes.data, f1.ctypes.data)
    counts = (ctypes.c_int32 * 2)(3, 1500)
    bank = ctypes.c_void_p()
    make = lib.bsrnn_fir_bank_create
    assert make(None, 2, ptrs, counts, ctypes.byref(bank)) == EARG
    assert make(host_ctx, 0, ptrs, counts, ctypes.byref(bank)) == EARG and "n_filters = 0" in err(), err()
    assert make(host_ctx, 2, None, counts, ctypes.byref(bank)) == EARG
    assert make(host_ctx, 2, ptrs, None, ctypes.byref(bank)) == EARG
    assert make(host_ctx, 2, ptrs, counts, None) == EARG
    assert make(host_ctx, 2, (ctypes.c_void_p * 2)(f0.ctypes.data, None), counts, ctypes.byref(bank)) == EARG and "taps_host[1]" in err(), err()
    for bad in (0, -3, 262145):
        assert make(host_ctx, 2, ptrs, (ctypes.c_int32 * 2)(3, bad), ctypes.byref(bank)) == EARG
        assert "n_taps_host[1] = %d" % bad in err() and "262144" in err(), err()
    assert not bank.value
    # a bank of a host-only context holds the tap counts and answers every refusal in front of BSRNN_ESTATE
    assert make(host_ctx, 2, ptrs, counts, ctypes.byref(bank)) == 0 and bank.value
    assert lib.bsrnn_fir_bank_count(bank) == 2 and lib.bsrnn_fir_bank_count(None) == -1
    assert [lib.bsrnn_fir_bank_taps(bank, i) for i in (-1, 0, 1, 2)] == [-1, 3, 1500, -1] and lib.bsrnn_fir_bank_taps(None, 0) == -1
    a, b = np.zeros((3, 100), np.float32), np.zeros((3, 100), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    i64s, i32s = (lambda *v: (ctypes.c_int64 * len(v))(*v)), (lambda *v: (ctypes.c_int32 * len(v))(*v))
    lens, filt = i64s(100, 50, 1), i32s(0, -1, 1)
    call = lib.bsrnn_convolve_ragged
    assert call(None, pa, 100, lens, filt, pb, 100, 3, None) == EARG and "null FIR bank" in err()
    for args in ((bank, None, 100, lens, filt, pb, 100, 3, None), (bank, pa, 100, None, filt, pb, 100, 3, None),
                 (bank, pa, 100, lens, None, pb, 100, 3, None), (bank, pa, 100, lens, filt, None, 100, 3, None)):
        assert call(*args) == EARG and "null argument" in err(), err()
    for R in (0, -2):
        assert call(bank, pa, 100, lens, filt, pb, 100, R, None) == EARG and "R = %d" % R in err(), err()
    for bad in (0, -7, (1 << 40) + 1):
        assert call(bank, pa, 1 << 41, i64s(100, bad, 1), filt, pb, 1 << 41, 3, None) == EARG
        assert "lens_host[1] = %d" % bad in err(), err()
    assert call(bank, pa, 99, lens, filt, pb, 100, 3, None) == EARG and "in_stride 99" in err() and "lens_host[0] = 100" in err(), err()
    assert call(bank, pa, 100, lens, filt, pb, 60, 3, None) == EARG and "out_stride 60" in err(), err()
    for bad in (2, -2):
        assert call(bank, pa, 100, lens, i32s(0, bad, 1), pb, 100, 3, None) == EARG
        assert "filter_host[1] = %d" % bad in err() and "[-1, 2)" in err(), err()
    assert call(bank, pa, 100, lens, filt, pa, 100, 3, None) == EARG and "overlap" in err(), err()
    tail = ctypes.c_void_p(pa.value + 4 * 200)                          # the one sample of the last row
    assert call(bank, pa, 100, lens, filt, tail, 100, 3, None) == EARG and "overlap" in err(), err()
    behind = ctypes.c_void_p(pa.value + 4 * 201)                        # the float behind it is not the input's
    assert call(bank, pa, 100, lens, filt, behind, 100, 1, None) == ESTATE
    # valid arguments: a host-only context cannot compute
    assert call(bank, pa, 100, lens, filt, pb, 100, 3, None) == ESTATE and "host-only" in err(), err()
    assert not a.any() and not b.any()
    lib.bsrnn_fir_bank_destroy(bank)
    lib.bsrnn_fir_bank_destroy(None)


def test_python_layer_signatures():
    import inspect
    from speechseparation_amd import augment
    assert list(inspect.signature(augment.FirBank.__init__).parameters) == ["self", "model", "filters"]
    sig = inspect.signature(augment.FirBank.convolve)
    assert list(sig.parameters) == ["self", "wave", "lengths", "filters", "out"]
    assert all(sig.parameters[p].default is None for p in ("lengths", "filters", "out"))
    assert callable(augment.FirBank.taps) and callable(augment.FirBank.__len__)
    assert list(inspect.signature(augment.rir_draw).parameters) == ["idx", "n_rirs", "channels_of", "prob"]
    assert inspect.signature(augment.rir_draw).parameters["prob"].default == 0.1
    sig = inspect.signature(augment.reverb_pairs)
    assert list(sig.parameters) == ["bank", "mixes", "draws", "chain"] and sig.parameters["chain"].default is True
    assert "m_dataset.py:111" in augment.reverb_pairs.__doc__
    assert list(inspect.signature(augment.remix).parameters) == ["dialog", "backgrounds", "length", "rng"]
