"""CPU-side tests of the native session pool's sessions at their own sample rates (bsrnn_pool_create_rates / _open_rate / _rate_of /
_ready / _drain_len / _drain, NativeRatePool): the declarations, the exports and the bindings, the refusals that need no pool, the Python
class's errors before a context exists, and the counts and capacities of csrc/pool_rates_host.h (through the small program
tests/cpp/pool_rates_check.cpp).  No compute here; tests/test_gpu_pool_native_rates.py holds the arithmetic."""
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
    "bsrnn_pool_create_rates": ("int", ["bsrnn_ctx*", "int32_t", "int32_t", "int32_t", "constint32_t*", "int32_t", "int64_t", "bsrnn_pool**"]),
    "bsrnn_pool_open_rate": ("int", ["bsrnn_pool*", "int32_t", "int32_t*"]),
    "bsrnn_pool_rate_of": ("int32_t", ["constbsrnn_pool*", "int32_t"]),
    "bsrnn_pool_ready": ("int64_t", ["constbsrnn_pool*", "int32_t", "int64_t"]),
    "bsrnn_pool_drain_len": ("int64_t", ["constbsrnn_pool*", "int32_t"]),
    "bsrnn_pool_drain": ("int", ["bsrnn_pool*", "int32_t", "float*", "int64_t", "int64_t*", "float", "void*"]),
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
    for name, (ret, want) in CALLS.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s*\b%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.M)
        assert m, name
        assert m.group(1).replace(" ", "") == ret, (name, m.group(1))
        types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert types == want, (name, types)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)          # additive: the version stays


def test_calls_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    for name in CALLS:
        assert name in exported and name in native.SYMBOLS, name
        assert getattr(native.lib, name).argtypes is not None, name
    lib = native.lib
    assert lib.bsrnn_pool_create_rates.argtypes == [vp, i32, i32, i32, vp, i32, i64, ctypes.POINTER(vp)]
    assert lib.bsrnn_pool_drain.argtypes == [vp, i32, vp, i64, ctypes.POINTER(i64), ctypes.c_float, vp]
    assert lib.bsrnn_pool_rate_of.restype == i32 and lib.bsrnn_pool_ready.restype == i64 and lib.bsrnn_pool_drain_len.restype == i64
    assert lib.bsrnn_abi_version() == 2


def test_a_null_pool_is_refused_by_every_call(native):
    lib = native.lib
    buf = (ctypes.c_float * 2048)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rates = (ctypes.c_int32 * 2)(16000, 48000)
    n = ctypes.c_int32(-5)
    got = ctypes.c_int64(-9)
    out = ctypes.c_void_p()

    def refused(rc, name):
        assert rc == EARG, name
        assert name.encode() in lib.bsrnn_last_error() and b"null" in lib.bsrnn_last_error(), lib.bsrnn_last_error()
    refused(lib.bsrnn_pool_create_rates(None, 4, 2, 3, rates, 2, 48000, ctypes.byref(out)), "bsrnn_pool_create_rates")
    assert out.value is None
    refused(lib.bsrnn_pool_open_rate(None, 48000, ctypes.byref(n)), "bsrnn_pool_open_rate")
    refused(lib.bsrnn_pool_drain(None, 0, p, 2048, ctypes.byref(got), ctypes.c_float(1.0), None), "bsrnn_pool_drain")
    assert n.value == -5 and got.value == -9                    # nothing was reported
    assert lib.bsrnn_pool_rate_of(None, 0) == -1
    assert lib.bsrnn_pool_ready(None, 0, 1024) == -1
    assert lib.bsrnn_pool_drain_len(None, 0) == -1


def test_python_class_offers_the_methods():
    from speechseparation_amd.bsrnn import NativeRatePool, NativeStreamPool
    import speechseparation_amd
    assert speechseparation_amd.NativeRatePool is NativeRatePool and issubclass(NativeRatePool, NativeStreamPool)
    sig = inspect.signature(NativeRatePool)
    assert list(sig.parameters) == ["model", "slots", "rows_per_session", "device", "max_hops", "rates", "max_block"]
    assert sig.parameters["rates"].default == (48000,) and sig.parameters["max_block"].default == 48000
    assert sig.parameters["rows_per_session"].default == 1 and sig.parameters["device"].default is None and sig.parameters["max_hops"].default == 8
    for name in ("open", "close", "sessions", "pending", "rate_of", "feed", "step", "drain", "export", "adopt"):
        assert callable(getattr(NativeRatePool, name)), name
    assert list(inspect.signature(NativeRatePool.feed).parameters) == ["self", "chunks", "mix"]
    assert list(inspect.signature(NativeRatePool.drain).parameters) == ["self", "sid", "mix"]
    assert list(inspect.signature(NativeRatePool.open).parameters) == ["self", "sample_rate"]
    # NativeStreamPool is what it was
    sig = inspect.signature(NativeStreamPool)
    assert list(sig.parameters) == ["model", "slots", "rows_per_session", "device", "max_hops"]
    assert sig.parameters["rows_per_session"].default == 1 and sig.parameters["device"].default is None and sig.parameters["max_hops"].default == 8


def test_rate_pool_checks_before_a_context_exists():
    import torch
    from speechseparation_amd.bsrnn import BSRNN, NativeRatePool
    m = BSRNN()
    for bad in (lambda: NativeRatePool(m, 0), lambda: NativeRatePool(m, 2, rows_per_session=0), lambda: NativeRatePool(m, 2, max_hops=256),
                lambda: NativeRatePool(m, 2, rates=None), lambda: NativeRatePool(m, 2, rates=()), lambda: NativeRatePool(m, 2, rates=48000),
                lambda: NativeRatePool(m, 2, rates=(48000.0,)), lambda: NativeRatePool(m, 2, rates=(True,)),
                lambda: NativeRatePool(m, 2, rates=(0,)), lambda: NativeRatePool(m, 2, rates=(44101,)),          # a ratio beyond the conversion's limit
                lambda: NativeRatePool(m, 2, rates=tuple(range(8000, 8017))),                                    # 17 rates
                lambda: NativeRatePool(m, 2, max_block=0), lambda: NativeRatePool(m, 2, max_block=2.5),
                lambda: NativeRatePool(m, 2, max_block=True), lambda: NativeRatePool(m, 2, max_block=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            bad()
    pool = NativeRatePool(m, 4, rows_per_session=2, max_hops=3, rates=(16000, 48000), max_block=4800)
    a, b, c = pool.open(sample_rate=48000), pool.open(), pool.open(sample_rate=16000)
    assert pool.sessions() == [a, b, c]
    assert [pool.rate_of(s) for s in (a, b, c)] == [48000, 44100, 16000]
    some = torch.zeros((2, 700))
    wide = torch.zeros((2, 2048))
    for bad, exc in ((lambda: pool.open(sample_rate=22050), ValueError),                        # a rate not declared
                     (lambda: pool.open(sample_rate="48000"), ValueError),
                     (lambda: pool.feed({a: some}), ValueError),                                # a CPU chunk of a session with a rate
                     (lambda: pool.feed({b: some, a: some}), ValueError),
                     (lambda: pool.feed({a: torch.zeros((1, 1024))}), ValueError),              # shapes
                     (lambda: pool.feed({a: torch.zeros(1024)}), ValueError),
                     (lambda: pool.feed({a: "chunk"}), ValueError),
                     (lambda: pool.feed([some]), ValueError),
                     (lambda: pool.feed({b: some.double()}), ValueError),                       # dtype
                     (lambda: pool.feed({b: wide[:, ::2]}), ValueError),                        # strides
                     (lambda: pool.feed({b: some}, mix="wet"), ValueError),
                     (lambda: pool.feed({77: some}), KeyError),
                     (lambda: pool.rate_of(77), KeyError),
                     (lambda: pool.drain(77), KeyError),
                     (lambda: pool.drain(a, mix="wet"), ValueError),
                     (lambda: pool.step({a: torch.zeros((2, 1024)), b: torch.zeros((2, 1024))}), ValueError),      # step: not for a rate
                     (lambda: pool.export(a), ValueError),
                     (lambda: pool.export(77), KeyError)):
        with pytest.raises(exc):
            bad()
    with pytest.raises(ValueError, match=r"feed\(\)"):
        pool.step({a: torch.zeros((2, 1024))})
    with pytest.raises(ValueError, match="max_block"):
        pool.feed({a: torch.zeros((2, 4801))})
    assert pool.feed({}) == {} and pool.step({}) == {}
    assert pool.pending(a) == 0
    # slots: the lowest free one; a closed session's rate goes with it
    pool.close(a)
    d = pool.open()
    assert pool._slot[d] == 0 and pool.rate_of(d) == 44100 and pool.sessions() == [b, c, d]
    e = pool.open(sample_rate=44100)
    assert pool.rate_of(e) == 44100
    with pytest.raises(ValueError):
        pool.open(sample_rate=16000)                                                            # every slot is taken
    assert m._ctx is None and pool._h is None


# ------------------------------------------------------------------------------------------------ the counts of pool_rates_host.h
def test_pool_rates_counts(tmp_path):
    exe = str(tmp_path / "pool_rates_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "pool_rates_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout


def test_pool_plan_check_still_passes_with_the_wider_entry(tmp_path):
    """PoolEntry grew by the scatter's first-segment offset; the plan's own check program, unchanged, still holds."""
    exe = str(tmp_path / "pool_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "pool_plan_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
