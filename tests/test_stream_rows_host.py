"""CPU-side tests of the streaming session slots (bsrnn_stream_process_rows / _reset_rows / _row_floats / _get_row / _set_row,
StreamingSeparator.process_rows / reset_rows / get_row / set_row, StreamPool): the declarations, the export and the binding, argument
checking without a GPU, the Python classes' errors before a context exists, and the row bitset of csrc/stream_rows_host.h (through
the small program tests/cpp/stream_rows_check.cpp).  No compute here; tests/test_gpu_stream_rows.py holds the arithmetic."""
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
SIGNATURES = {
    "bsrnn_stream_process_rows": ("int", ["bsrnn_stream*", "constfloat*", "float*", "int32_t", "constuint8_t*", "constfloat*", "float", "void*"]),
    "bsrnn_stream_reset_rows": ("int", ["bsrnn_stream*", "constint32_t*", "int32_t", "void*"]),
    "bsrnn_stream_row_floats": ("int64_t", ["constbsrnn_stream*"]),
    "bsrnn_stream_get_row": ("int", ["bsrnn_stream*", "int32_t", "float*"]),
    "bsrnn_stream_set_row": ("int", ["bsrnn_stream*", "int32_t", "constfloat*"]),
}


@pytest.fixture(scope="module")
def native():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd import _native
    return _native


def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, (ret, args) in SIGNATURES.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert types == args, (name, types)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)
    assert re.search(r"#define\s+BSRNN_STREAM_ROWS_MAX\s+2048\b", txt)


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in SIGNATURES:
        assert name in native.SYMBOLS, name
        assert name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib = native.lib
    assert lib.bsrnn_stream_process_rows.argtypes == [vp, vp, vp, i32, vp, vp, ctypes.c_float, vp]
    assert lib.bsrnn_stream_reset_rows.argtypes == [vp, vp, i32, vp]
    assert lib.bsrnn_stream_row_floats.argtypes == [vp] and lib.bsrnn_stream_row_floats.restype == i64
    assert lib.bsrnn_stream_get_row.argtypes == [vp, i32, vp]
    assert lib.bsrnn_stream_set_row.argtypes == [vp, i32, vp]
    for name in ("bsrnn_stream_process_rows", "bsrnn_stream_reset_rows", "bsrnn_stream_get_row", "bsrnn_stream_set_row"):
        assert getattr(lib, name).restype == ctypes.c_int
    assert native.STREAM_ROWS_MAX == 2048
    assert lib.bsrnn_abi_version() == 2


def test_null_arguments_are_refused_without_a_gpu(native):
    lib = native.lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rows = (ctypes.c_int32 * 2)(0, 1)
    flags = (ctypes.c_uint8 * 2)(1, 0)

    def refused(rc, name):
        assert rc == EARG, name
        assert name.encode() in lib.bsrnn_last_error(), lib.bsrnn_last_error()
    refused(lib.bsrnn_stream_process_rows(None, p, p, 1, flags, None, ctypes.c_float(1.0), None), "bsrnn_stream_process_rows")
    refused(lib.bsrnn_stream_process_rows(None, p, p, 0, None, None, ctypes.c_float(1.0), None), "bsrnn_stream_process_rows")
    refused(lib.bsrnn_stream_process_rows(None, None, None, 1, None, None, ctypes.c_float(1.0), None), "bsrnn_stream_process_rows")
    refused(lib.bsrnn_stream_reset_rows(None, rows, 2, None), "bsrnn_stream_reset_rows")
    refused(lib.bsrnn_stream_reset_rows(None, None, 0, None), "bsrnn_stream_reset_rows")
    refused(lib.bsrnn_stream_get_row(None, 0, p), "bsrnn_stream_get_row")
    refused(lib.bsrnn_stream_set_row(None, 0, p), "bsrnn_stream_set_row")
    assert lib.bsrnn_stream_row_floats(None) == -1
    assert list(flags) == [1, 0] and list(rows) == [0, 1]        # the caller's arrays: read at most, never written


def test_python_classes_offer_the_methods():
    from speechseparation_amd.bsrnn import StreamingSeparator, StreamPool
    assert list(inspect.signature(StreamingSeparator.process_rows).parameters) == ["self", "wave", "active", "mix"]
    sig = inspect.signature(StreamingSeparator.process_rows)
    assert sig.parameters["active"].default is None and sig.parameters["mix"].default == 1.0
    assert list(inspect.signature(StreamingSeparator.reset_rows).parameters) == ["self", "rows"]
    assert list(inspect.signature(StreamingSeparator.get_row).parameters) == ["self", "row"]
    assert list(inspect.signature(StreamingSeparator.set_row).parameters) == ["self", "row", "blob"]
    for name in ("step", "process", "reset", "state"):
        assert callable(getattr(StreamingSeparator, name, None)), name
    sig = inspect.signature(StreamPool.__init__)
    assert list(sig.parameters) == ["self", "model", "slots", "rows_per_session", "device", "rates"]
    assert sig.parameters["rows_per_session"].default == 1 and sig.parameters["device"].default is None and sig.parameters["rates"].default is None
    assert list(inspect.signature(StreamPool.step).parameters) == ["self", "chunks", "mix"]
    assert inspect.signature(StreamPool.step).parameters["mix"].default is None
    for name in ("open", "close", "export", "adopt"):
        assert callable(getattr(StreamPool, name, None)), name


def test_stream_pool_checks_before_a_context_exists():
    import torch
    from speechseparation_amd.bsrnn import BSRNN, StreamPool
    m = BSRNN()
    pool = StreamPool(m, 2, rows_per_session=2)
    a, b = pool.open(), pool.open()
    assert a != b
    with pytest.raises(ValueError):
        pool.open()                                                            # full
    hop = torch.zeros((2, 1024))
    for bad, exc in ((lambda: pool.step({a: hop, b: torch.zeros((2, 2048))}), ValueError),      # unequal L
                     (lambda: pool.step({a: torch.zeros((1, 1024))}), ValueError),              # a wrong row count
                     (lambda: pool.step({a: torch.zeros((2, 1000))}), ValueError),              # no whole hops
                     (lambda: pool.step({a: torch.zeros(1024)}), ValueError),
                     (lambda: pool.step({a: "chunk"}), ValueError),
                     (lambda: pool.step([hop]), ValueError),
                     (lambda: pool.step({a: hop}, mix="wet"), ValueError),
                     (lambda: pool.step({a: hop}, mix={a: "wet"}), ValueError),
                     (lambda: pool.step({a: hop}, mix={77: 0.5}), KeyError),
                     (lambda: pool.step({77: hop}), KeyError),                                  # an unknown session
                     (lambda: pool.export(77), KeyError),
                     (lambda: pool.close(77), KeyError),
                     (lambda: pool.adopt([torch.zeros(5)] * 2), ValueError),
                     (lambda: pool.adopt([torch.zeros(2 * 2048 + 8 * len(m.band_widths) * 64)]), ValueError)):
        with pytest.raises(exc):
            bad()
    assert pool.step({}) == {}                                                 # nobody has audio: no library call
    pool.close(a)
    c = pool.open()                                                            # the freed slot is taken again
    assert c not in (a, b) and sorted(pool.sessions()) == sorted([b, c])
    with pytest.raises(ValueError):
        pool.open()
    with pytest.raises(KeyError):
        pool.step({a: hop})                                                    # closed
    for bad in (lambda: StreamPool(m, 0), lambda: StreamPool(m, 2, rows_per_session=0), lambda: StreamPool(m, 2.5),
                lambda: StreamPool(m, 1025, rows_per_session=2)):
        with pytest.raises(ValueError):
            bad()
    assert m._ctx is None and pool._st is None


# ------------------------------------------------------------------------------------------------ the row bitset of stream_rows_host.h
def test_row_bitset(tmp_path):
    exe = str(tmp_path / "stream_rows_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "stream_rows_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
