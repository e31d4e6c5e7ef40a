"""Block streaming (bsrnn_stream_process / bsrnn_stream_reserve): what can be checked without a GPU - the two symbols are
declared, listed and exported together, refuse null arguments before touching the device, and the Python class offers them."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bsrnn_hip.h")
NEW = ("bsrnn_stream_process", "bsrnn_stream_reserve")
BSRNN_EARG = 1


def test_symbols_declared_listed_and_exported():
    from speechseparation_amd import _native
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(bsrnn_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared, name
        assert name in _native.SYMBOLS, name
        assert hasattr(ctypes.CDLL(_native.LIB_PATH), name), name
    assert re.search(r"int\s+bsrnn_stream_process\(bsrnn_stream\*\s*\w+,\s*const float\*\s*\w+,\s*float\*\s*\w+,\s*int32_t\s+\w+,\s*float\s+\w+,\s*void\*\s*\w+\);", text)
    assert re.search(r"int\s+bsrnn_stream_reserve\(bsrnn_stream\*\s*\w+,\s*int32_t\s+\w+\);", text)
    assert _native.lib.bsrnn_abi_version() == 2


def test_null_stream_is_refused_without_a_gpu():
    from speechseparation_amd import _native
    lib = _native.lib
    buf = (ctypes.c_float * 2048)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.bsrnn_stream_process(None, p, p, 1, ctypes.c_float(1.0), None) == BSRNN_EARG
    assert b"bsrnn_stream_process" in lib.bsrnn_last_error()
    assert lib.bsrnn_stream_reserve(None, 1) == BSRNN_EARG
    assert b"bsrnn_stream_reserve" in lib.bsrnn_last_error()


def test_python_class_offers_process_and_reserve():
    from speechseparation_amd.bsrnn import StreamingSeparator
    assert callable(getattr(StreamingSeparator, "process", None))
    assert callable(getattr(StreamingSeparator, "reserve", None))
    assert callable(getattr(StreamingSeparator, "step", None))
