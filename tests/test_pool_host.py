"""CPU-side tests of the native session pool (bsrnn_pool_*, NativeStreamPool): the declarations, the exports and the bindings, the
refusals that need no pool, the Python class's errors before a context exists, and the slots / pending counts / round plan of
csrc/pool_host.h (through the small program tests/cpp/pool_plan_check.cpp).  No compute here; tests/test_gpu_pool_native.py holds the
arithmetic."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
EARG = 1                     # BSRNN_EARG of include/bsrnn_hip.h
CALLS = {                    # name -> (return type, parameter types) as the header declares them
    "bsrnn_pool_create": ("int", ["bsrnn_ctx*", "int32_t", "int32_t", "int32_t", "bsrnn_pool**"]),
    "bsrnn_pool_destroy": ("void", ["bsrnn_pool*"]),
    "bsrnn_pool_open": ("int", ["bsrnn_pool*", "int32_t*"]),
    "bsrnn_pool_close": ("int", ["bsrnn_pool*", "int32_t"]),
    "bsrnn_pool_pending": ("int64_t", ["constbsrnn_pool*", "int32_t"]),
    "bsrnn_pool_stream": ("bsrnn_stream*", ["bsrnn_pool*"]),
    "bsrnn_pool_get_pending": ("int", ["bsrnn_pool*", "int32_t", "float*", "int32_t*"]),
    "bsrnn_pool_set_pending": ("int", ["bsrnn_pool*", "int32_t", "constfloat*", "int32_t"]),
    "bsrnn_pool_feed": ("int", ["bsrnn_pool*", "int32_t", "constint32_t*", "constfloat*const*", "constint64_t*", "constint64_t*",
                                "float*const*", "constint64_t*", "int64_t*", "constfloat*", "float", "void*"]),
    "bsrnn_pool_feed_host": ("int", ["bsrnn_pool*", "int32_t", "constint32_t*", "constfloat*const*", "constint64_t*", "constint64_t*",
                                     "float*const*", "constint64_t*", "int64_t*", "constfloat*", "float"]),
}


@pytest.fixture(scope="module")
def native():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd import _native
    return _native


def test_header_declares_the_calls():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef\s+struct\s+bsrnn_pool\s+bsrnn_pool\s*;", txt)
    for name, (ret, want) in CALLS.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.M)
        assert m, name
        assert m.group(1).replace(" ", "") == ret, (name, m.group(1))
        types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert types == want, (name, types)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)


def test_calls_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for name in CALLS:
        assert name in exported and name in native.SYMBOLS, name
        assert getattr(native.lib, name).argtypes is not None, name
    assert native.lib.bsrnn_pool_feed.argtypes == [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_float, vp]
    assert native.lib.bsrnn_pool_feed_host.argtypes == [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_float]
    assert native.lib.bsrnn_pool_pending.restype == i64 and native.lib.bsrnn_pool_stream.restype == vp
    assert native.lib.bsrnn_abi_version() == 2


def test_a_null_pool_is_refused_by_every_call(native):
    lib = native.lib
    buf = (ctypes.c_float * 2048)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = ctypes.c_float(1.0)
    n = ctypes.c_int32(-5)
    slots = (ctypes.c_int32 * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(p.value)
    cnt = (ctypes.c_int64 * 1)(1024)
    got = (ctypes.c_int64 * 1)(-9)
    out = ctypes.c_void_p()

    def refused(rc, name):
        assert rc == EARG, name
        assert name.encode() in lib.bsrnn_last_error() and b"null" in lib.bsrnn_last_error(), lib.bsrnn_last_error()
    refused(lib.bsrnn_pool_create(None, 4, 2, 3, ctypes.byref(out)), "bsrnn_pool_create")
    assert out.value is None
    refused(lib.bsrnn_pool_open(None, ctypes.byref(n)), "bsrnn_pool_open")
    refused(lib.bsrnn_pool_close(None, 0), "bsrnn_pool_close")
    refused(lib.bsrnn_pool_get_pending(None, 0, p, ctypes.byref(n)), "bsrnn_pool_get_pending")
    refused(lib.bsrnn_pool_set_pending(None, 0, p, 5), "bsrnn_pool_set_pending")
    refused(lib.bsrnn_pool_feed(None, 1, slots, ptrs, cnt, cnt, ptrs, cnt, got, None, one, None), "bsrnn_pool_feed")
    refused(lib.bsrnn_pool_feed_host(None, 1, slots, ptrs, cnt, cnt, ptrs, cnt, got, None, one), "bsrnn_pool_feed_host")
    refused(lib.bsrnn_pool_feed(None, 0, None, None, None, None, None, None, None, None, one, None), "bsrnn_pool_feed")
    assert n.value == -5 and got[0] == -9                       # nothing was reported
    assert lib.bsrnn_pool_pending(None, 0) == -1
    assert lib.bsrnn_pool_stream(None) is None
    lib.bsrnn_pool_destroy(None)                                # ignored, as the other destroy calls ignore a null handle


def test_python_class_offers_the_methods():
    from speechseparation_amd.bsrnn import NativeStreamPool, StreamPool
    import speechseparation_amd
    assert speechseparation_amd.NativeStreamPool is NativeStreamPool
    sig = inspect.signature(NativeStreamPool)
    assert list(sig.parameters) == ["model", "slots", "rows_per_session", "device", "max_hops"]
    assert sig.parameters["rows_per_session"].default == 1 and sig.parameters["device"].default is None and sig.parameters["max_hops"].default == 8
    for name in ("open", "close", "sessions", "pending", "feed", "step", "export", "adopt"):
        assert callable(getattr(NativeStreamPool, name)), name
    sig = inspect.signature(NativeStreamPool.feed)
    assert list(sig.parameters) == ["self", "chunks", "mix"] and sig.parameters["mix"].default is None
    assert list(inspect.signature(NativeStreamPool.step).parameters) == ["self", "chunks", "mix"]
    # StreamPool is what it was
    assert list(inspect.signature(StreamPool).parameters) == ["model", "slots", "rows_per_session", "device", "rates"]


def test_native_pool_checks_before_a_context_exists():
    import torch
    from speechseparation_amd.bsrnn import BSRNN, NativeStreamPool
    m = BSRNN()
    for bad in (lambda: NativeStreamPool(m, 0), lambda: NativeStreamPool(m, 2, rows_per_session=0), lambda: NativeStreamPool(m, True),
                lambda: NativeStreamPool(m, 2.0), lambda: NativeStreamPool(m, 2048, rows_per_session=2),
                lambda: NativeStreamPool(m, 2, max_hops=0), lambda: NativeStreamPool(m, 2, max_hops=256)):
        with pytest.raises(ValueError):
            bad()
    pool = NativeStreamPool(m, 3, rows_per_session=2, max_hops=3)
    a, b = pool.open(), pool.open()
    assert pool.sessions() == [a, b]
    some = torch.zeros((2, 700))
    wide = torch.zeros((2, 2048))
    for bad, exc in ((lambda: pool.feed({a: torch.zeros((1, 1024))}), ValueError),              # shapes
                     (lambda: pool.feed({a: torch.zeros((3, 10))}), ValueError),
                     (lambda: pool.feed({a: torch.zeros(1024)}), ValueError),
                     (lambda: pool.feed({a: "chunk"}), ValueError),
                     (lambda: pool.feed([some]), ValueError),
                     (lambda: pool.feed({a: some.double()}), ValueError),                       # a dtype that cannot go by pointer
                     (lambda: pool.feed({a: some.to(torch.int32)}), ValueError),
                     (lambda: pool.feed({a: wide[:, ::2]}), ValueError),                        # strides that cannot go by pointer
                     (lambda: pool.feed({a: torch.zeros((700, 2)).t()}), ValueError),
                     (lambda: pool.feed({a: torch.zeros((1, 700)).expand(2, 700)}), ValueError),
                     (lambda: pool.feed({a: some}, mix="wet"), ValueError),                     # bad mix
                     (lambda: pool.feed({a: some}, mix=True), ValueError),
                     (lambda: pool.feed({a: some}, mix={a: "wet"}), ValueError),
                     (lambda: pool.feed({a: some}, mix={77: 0.5}), KeyError),
                     (lambda: pool.feed({77: some}), KeyError),                                 # an unknown session
                     (lambda: pool.pending(77), KeyError),
                     (lambda: pool.close(77), KeyError),
                     (lambda: pool.export(77), KeyError),
                     (lambda: pool.step({a: some}), ValueError),                                # step: whole equal hops
                     (lambda: pool.step({a: torch.zeros((2, 0))}), ValueError),
                     (lambda: pool.step({a: torch.zeros((2, 1024)), b: torch.zeros((2, 2048))}), ValueError),
                     (lambda: pool.step({77: torch.zeros((2, 1024))}), KeyError),
                     (lambda: pool.step([wide]), ValueError),
                     (lambda: pool.adopt([torch.zeros(5)] * 2), ValueError),
                     (lambda: pool.adopt([torch.zeros(5)]), ValueError),
                     (lambda: pool.open(sample_rate=48000), ValueError),                        # rates are StreamPool's
                     (lambda: pool.open(sample_rate=16000), ValueError)):
        with pytest.raises(exc):
            bad()
    with pytest.raises(ValueError, match=r"StreamPool\(rates="):
        pool.open(sample_rate=48000)
    assert pool.feed({}) == {} and pool.step({}) == {}                          # nobody named: no library call
    assert pool.pending(a) == 0 and pool.pending(b) == 0
    # slots: the lowest free one, as the library hands them out
    c = pool.open(sample_rate=44100)
    with pytest.raises(ValueError):
        pool.open()
    pool.close(a)
    d = pool.open()
    assert pool._slot[d] == 0 and pool._slot[b] == 1 and pool._slot[c] == 2 and pool.sessions() == [b, c, d]
    assert m._ctx is None and pool._h is None


# ------------------------------------------------------------------------------------------------ the plan of pool_host.h
def test_pool_plan(tmp_path):
    exe = str(tmp_path / "pool_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "pool_plan_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
