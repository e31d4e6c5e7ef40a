"""CPU-side tests of the long-form separation interface (bsrnn_separate_long, bsrnn_separate_long_host, bsrnn_workspace_rows):
declarations, exports, argument checking on a host-only context, the Python methods and the infer.py flag.  No compute here;
tests/test_gpu_separate_long.py holds the arithmetic."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from speechseparation_amd import spec

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
NEW = ("bsrnn_separate_long", "bsrnn_separate_long_host", "bsrnn_workspace_rows")


@pytest.fixture(scope="module")
def native():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd import _native
    return _native


@pytest.fixture()
def host_ctx(native):
    v = spec.generate_bandsplits()[0]
    ctx = ctypes.c_void_p()
    assert native.lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(ctx)) == 0
    yield ctx
    native.lib.bsrnn_destroy(ctx)


def declarations():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(2): (m.group(1).strip(), re.sub(r"\s+", " ", m.group(3)).strip())
            for m in re.finditer(r"^\s*([A-Za-z_][\w \*]*?)\s+\**(bsrnn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt, flags=re.M)}


def types_of(params):
    """The parameter types of a C parameter list, names and spaces dropped."""
    return [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in params.split(",")]


def test_header_declares_the_three_symbols():
    d = declarations()
    assert d["bsrnn_separate_long"][0] == "int"
    assert types_of(d["bsrnn_separate_long"][1]) == ["bsrnn_ctx*", "constfloat*", "float*", "int32_t", "int64_t", "int32_t", "void*"]
    assert d["bsrnn_separate_long_host"][0] == "int"
    assert types_of(d["bsrnn_separate_long_host"][1]) == ["bsrnn_ctx*", "constfloat*", "float*", "int32_t", "int64_t", "int32_t"]
    assert d["bsrnn_workspace_rows"][0] == "int64_t"
    assert types_of(d["bsrnn_workspace_rows"][1]) == ["constbsrnn_ctx*"]


def test_symbols_are_listed_bound_and_exported(native):
    for s in NEW:
        assert s in native.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_separate_long.argtypes == [vp, vp, vp, i32, i64, i32, vp]
    assert native.lib.bsrnn_separate_long_host.argtypes == [vp, vp, vp, i32, i64, i32]
    assert native.lib.bsrnn_workspace_rows.argtypes == [vp] and native.lib.bsrnn_workspace_rows.restype == i64
    assert native.lib.bsrnn_abi_version() == 2


def test_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib
    n = 4 * 1024 + 5
    a, b = np.zeros((2, n), np.float32), np.zeros((2, 4 * 1024), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    # null context, null buffers
    assert lib.bsrnn_separate_long(None, pa, pb, 2, n, 2, None) == EARG
    assert lib.bsrnn_separate_long_host(None, pa, pb, 2, n, 2) == EARG
    assert lib.bsrnn_separate_long(host_ctx, None, pb, 2, n, 2, None) == EARG
    assert lib.bsrnn_separate_long(host_ctx, pa, None, 2, n, 2, None) == EARG
    assert lib.bsrnn_separate_long_host(host_ctx, None, pb, 2, n, 2) == EARG
    assert lib.bsrnn_separate_long_host(host_ctx, pa, None, 2, n, 2) == EARG
    # a host-only context cannot compute
    assert lib.bsrnn_separate_long(host_ctx, pa, pb, 2, n, 2, None) == ESTATE
    assert b"host-only" in lib.bsrnn_last_error()
    assert lib.bsrnn_separate_long_host(host_ctx, pa, pb, 2, n, 2) == ESTATE
    assert b"host-only" in lib.bsrnn_last_error()
    assert not a.any() and not b.any()


def test_workspace_rows_without_a_device(native, host_ctx):
    assert native.lib.bsrnn_workspace_rows(host_ctx) == 0
    assert native.lib.bsrnn_workspace_rows(None) == 0


def test_python_methods_exist(native):
    from speechseparation_amd.bsrnn import BSRNN
    sig = inspect.signature(BSRNN.separate_long)
    assert list(sig.parameters) == ["self", "waveform", "segment_frames", "out"]
    assert sig.parameters["segment_frames"].default == 256 and sig.parameters["out"].default is None
    assert list(inspect.signature(BSRNN.workspace_rows).parameters) == ["self", "device"]
    m = BSRNN()
    assert m.workspace_rows() == 0                        # no native context yet
    import torch
    with pytest.raises(ValueError):
        m.separate_long(torch.zeros(5000))                # a shape error, before any device is asked for


def test_infer_parser_accepts_segment_frames(native, capsys):
    import infer
    with pytest.raises(SystemExit) as e:
        infer.main(["--help"])
    assert e.value.code == 0 and "--segment-frames" in capsys.readouterr().out
    # the flag takes an integer: argparse refuses anything else before a model is built
    with pytest.raises(SystemExit) as e:
        infer.main(["--input", "a.wav", "--output", "b.wav", "--segment-frames", "many"])
    assert e.value.code == 2 and "--segment-frames" in capsys.readouterr().err
