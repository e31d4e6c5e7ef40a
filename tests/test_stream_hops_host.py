"""CPU-side tests of the hop count per row (bsrnn_stream_process_hops, StreamingSeparator.process_hops, StreamPool.feed / pending): the
declaration, the export and the binding, the refusals that need no stream, the Python classes' errors before a context exists, feeds
that make no library call, and the count table of csrc/stream_rows_host.h (through the small program tests/cpp/stream_hops_check.cpp).
No compute here; tests/test_gpu_stream_hops.py holds the arithmetic."""
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
NAME = "bsrnn_stream_process_hops"


@pytest.fixture(scope="module")
def native():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd import _native
    return _native


def test_header_declares_the_call():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % NAME, txt, flags=re.M)
    assert m and m.group(1).strip() == "int"
    types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
    assert types == ["bsrnn_stream*", "constfloat*", "float*", "int32_t", "constint32_t*", "constfloat*", "float", "void*"]
    assert re.search(r"#define\s+BSRNN_STREAM_HOPS_MAX\s+255\b", txt)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)


def test_call_is_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert NAME in set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    assert NAME in native.SYMBOLS
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    fn = getattr(native.lib, NAME)
    assert fn.argtypes == [vp, vp, vp, i32, vp, vp, ctypes.c_float, vp] and fn.restype == ctypes.c_int
    assert native.STREAM_HOPS_MAX == 255


def test_refusals_without_a_gpu(native):
    lib = native.lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    hops = (ctypes.c_int32 * 2)(1, 0)
    one = ctypes.c_float(1.0)

    def refused(rc, *words):
        assert rc == EARG
        for w in (NAME,) + words:
            assert w.encode() in lib.bsrnn_last_error(), lib.bsrnn_last_error()
    # a null pointer (no stream handle here, so every call below is answered before a device is touched)
    refused(lib.bsrnn_stream_process_hops(None, p, p, 1, hops, None, one, None), "null")
    refused(lib.bsrnn_stream_process_hops(None, None, None, 2, None, None, one, None), "null")
    refused(lib.bsrnn_stream_process_hops(None, p, p, 255, None, None, one, None), "null")
    # n_hops outside [1, BSRNN_STREAM_HOPS_MAX]
    for n in (0, -3, 256, 100000):
        refused(lib.bsrnn_stream_process_hops(None, p, p, n, hops, None, one, None), "n_hops = %d" % n, "255")
    assert list(hops) == [1, 0]                                  # the caller's array: read at most, never written


def test_python_classes_offer_the_methods():
    from speechseparation_amd.bsrnn import StreamingSeparator, StreamPool
    sig = inspect.signature(StreamingSeparator.process_hops)
    assert list(sig.parameters) == ["self", "wave", "hops", "mix"] and sig.parameters["mix"].default == 1.0
    sig = inspect.signature(StreamPool.feed)
    assert list(sig.parameters) == ["self", "chunks", "mix"] and sig.parameters["mix"].default is None
    assert list(inspect.signature(StreamPool.pending).parameters) == ["self", "sid"]
    # StreamPool.step is what it was
    sig = inspect.signature(StreamPool.step)
    assert list(sig.parameters) == ["self", "chunks", "mix"] and sig.parameters["mix"].default is None
    assert "export" in StreamPool.feed.__doc__ and "NOT part of the carry" in StreamPool.feed.__doc__     # the blob carries no pending samples


def test_process_hops_checks_its_arguments_first():
    """Argument errors are raised before any library call: the object below has no stream handle at all."""
    import torch
    from speechseparation_amd.bsrnn import StreamingSeparator
    st = object.__new__(StreamingSeparator)
    st.C = 3
    wave = torch.zeros((3, 2 * 1024))
    for bad in (lambda: st.process_hops(torch.zeros((2, 2048)), [1, 1, 1]),             # a wrong row count
                lambda: st.process_hops(torch.zeros(2048), [1, 1, 1]),
                lambda: st.process_hops("wave", [1, 1, 1]),
                lambda: st.process_hops(torch.zeros((3, 2000)), [1, 1, 1]),             # no whole hops
                lambda: st.process_hops(torch.zeros((3, 256 * 1024)), [1, 1, 1]),       # more than 255 hops
                lambda: st.process_hops(wave, [1, 1]),                                  # a wrong number of counts
                lambda: st.process_hops(wave, [1, 1, 1, 1]),
                lambda: st.process_hops(wave, [1, 3, 1]),                               # counts outside [0, L]
                lambda: st.process_hops(wave, [1, -1, 1]),
                lambda: st.process_hops(wave, torch.tensor([0, 0, 5])),
                lambda: st.process_hops(wave, [1, 1.5, 1]),
                lambda: st.process_hops(wave, [1, True, 1]),
                lambda: st.process_hops(wave, 2),
                lambda: st.process_hops(wave, [1, 1, 1], mix="wet"),                    # bad mix
                lambda: st.process_hops(wave, [1, 1, 1], mix=torch.ones(2)),
                lambda: st.process_hops(wave, [1, 1, 1], mix=True)):
        with pytest.raises(ValueError):
            bad()
    st._h = None          # (so that __del__ has something to hand to the library, which ignores a null handle)


def test_stream_pool_feed_checks_before_a_context_exists():
    import torch
    from speechseparation_amd.bsrnn import BSRNN, StreamPool
    m = BSRNN()
    pool = StreamPool(m, 2, rows_per_session=2)
    a, b = pool.open(), pool.open()
    some = torch.zeros((2, 700))
    for bad, exc in ((lambda: pool.feed({a: torch.zeros((1, 1024))}), ValueError),              # a wrong row count
                     (lambda: pool.feed({a: torch.zeros((3, 10))}), ValueError),
                     (lambda: pool.feed({a: torch.zeros(1024)}), ValueError),
                     (lambda: pool.feed({a: "chunk"}), ValueError),
                     (lambda: pool.feed([some]), ValueError),
                     (lambda: pool.feed({a: some}, mix="wet"), ValueError),                     # bad mix
                     (lambda: pool.feed({a: some}, mix=True), ValueError),
                     (lambda: pool.feed({a: some}, mix={a: "wet"}), ValueError),
                     (lambda: pool.feed({a: some}, mix={77: 0.5}), KeyError),
                     (lambda: pool.feed({77: some}), KeyError),                                 # an unknown session
                     (lambda: pool.pending(77), KeyError)):
        with pytest.raises(exc):
            bad()
    assert pool.pending(a) == 0 and pool.pending(b) == 0                       # a refused feed keeps nothing
    # nobody has audio, or nobody reaches a hop: no library call (there is no stream to make one on), the samples wait
    assert pool.feed({}) == {}
    x = torch.arange(2 * 1100, dtype=torch.float32).reshape(2, 1100)
    out = pool.feed({a: x[:, :700], b: torch.zeros((2, 0))})
    assert sorted(out) == sorted([a, b])
    assert all(tuple(o.shape) == (2, 0) and o.dtype == torch.float32 for o in out.values())
    assert pool.pending(a) == 700 and pool.pending(b) == 0
    out = pool.feed({a: x[:, 700:1000], b: x[:, :1023]}, mix={a: 0.5})
    assert all(tuple(o.shape) == (2, 0) for o in out.values())
    assert pool.pending(a) == 1000 and pool.pending(b) == 1023
    assert torch.equal(pool._pend[a], x[:, :1000])                             # in the order they came
    assert m._ctx is None and pool._st is None
    # close drops what waits; the slot's next session starts with nothing
    pool.close(a)
    with pytest.raises(KeyError):
        pool.pending(a)
    c = pool.open()
    assert pool.pending(c) == 0 and pool.pending(b) == 1023
    assert m._ctx is None and pool._st is None


# ------------------------------------------------------------------------------------------------ the count table of stream_rows_host.h
def test_row_hops_table(tmp_path):
    exe = str(tmp_path / "stream_hops_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "stream_hops_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
