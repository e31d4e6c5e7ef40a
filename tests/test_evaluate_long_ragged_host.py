"""CPU-side tests of the ragged long-form evaluate (bsrnn_evaluate_long_ragged, BSRNN.evaluate_long_ragged / evaluate_long /
evaluate_many_long, metrics.evaluate_many_long, validate.py --segment-frames): the declaration, the export and the binding, argument
checking on a host-only context, the Python methods' signatures and errors, and - through the small program
tests/cpp/evaluate_long_check.cpp, built with the address and undefined-behaviour sanitizers - which hops and frames a segment owns
(plan_host.h: segment_owned) and the SI-SDR sums formed from a row's totals (metrics_host.h: sisdr_sums_from_totals).  No compute here;
tests/test_gpu_evaluate_long_ragged.py holds the arithmetic."""
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
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
LENS = [9 * 1024 + 77, 3 * 1024 + 5, 4 * 1024, 7 * 1024 + 1023, 1500]
ROWS = [2, 1, 2, 2, 3]
STRIDE = 9 * 1024 + 77


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


def test_header_declares_the_symbol():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+bsrnn_evaluate_long_ragged\s*\(([^)]*)\)\s*;", txt, flags=re.M)
    assert m and m.group(1).strip() == "int"
    params = [p.strip() for p in m.group(2).split(",")]
    types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p).replace(" ", "") for p in params]
    assert types == ["bsrnn_ctx*", "constfloat*", "constfloat*", "int64_t", "constint64_t*", "constint32_t*", "int32_t", "int32_t", "float*",
                     "double*", "void*"]
    assert [re.search(r"([a-zA-Z_]\w*)$", p).group(1) for p in params] == [
        "ctx", "mix_dev", "speech_dev", "wave_stride", "clip_lens_host", "clip_rows_host", "n_clips", "seg_frames", "est_out_dev",
        "metrics_host", "stream"]
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)


def test_symbol_is_listed_bound_and_exported(native):
    assert "bsrnn_evaluate_long_ragged" in native.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "bsrnn_evaluate_long_ragged" in set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_evaluate_long_ragged.argtypes == [vp, vp, vp, i64, vp, vp, i32, i32, vp, ctypes.POINTER(ctypes.c_double), vp]
    assert native.lib.bsrnn_evaluate_long_ragged.restype == ctypes.c_int
    assert native.lib.bsrnn_abi_version() == 2


def test_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib
    R = sum(ROWS)
    a, b = np.zeros((R, STRIDE), np.float32), np.zeros((R, STRIDE), np.float32)
    e = np.zeros((R, 9 * 1024), np.float32)
    pa, pb, pe = (x.ctypes.data_as(ctypes.c_void_p) for x in (a, b, e))
    vals = (ctypes.c_double * (5 * 8))()

    def lens(values):
        return (ctypes.c_int64 * len(values))(*values)

    def rows(values):
        return (ctypes.c_int32 * len(values))(*values)

    def err():
        return lib.bsrnn_last_error().decode()
    gl, gr = lens(LENS), rows(ROWS)
    call = lib.bsrnn_evaluate_long_ragged
    # each null argument, and no clips
    assert call(None, pa, pb, STRIDE, gl, gr, 5, 3, pe, vals, None) == EARG
    assert call(host_ctx, None, pb, STRIDE, gl, gr, 5, 3, pe, vals, None) == EARG
    assert call(host_ctx, pa, None, STRIDE, gl, gr, 5, 3, pe, vals, None) == EARG
    assert call(host_ctx, pa, pb, STRIDE, None, gr, 5, 3, pe, vals, None) == EARG
    assert call(host_ctx, pa, pb, STRIDE, gl, gr, 5, 3, pe, None, None) == EARG
    assert call(host_ctx, pa, pb, STRIDE, gl, gr, 0, 3, pe, vals, None) == EARG
    assert call(host_ctx, pa, pb, STRIDE, gl, gr, -1, 3, pe, vals, None) == EARG
    # no frames in a segment
    for seg in (0, -5):
        assert call(host_ctx, pa, pb, STRIDE, gl, gr, 5, seg, pe, vals, None) == EARG
        assert "seg_frames" in err() and str(seg) in err(), err()
    # what bsrnn_evaluate_ragged refuses, in its words: the text names the clip and the value
    for seg in (3, 256):
        assert call(host_ctx, pa, pb, STRIDE, gl, rows([2, 1, 0, 2, 3]), 5, seg, pe, vals, None) == EARG
        assert re.search(r"\bclip 2\b", err()) and re.search(r"\b0 rows\b", err()), err()
        assert call(host_ctx, pa, pb, STRIDE, gl, rows([2, 1, 2, -3, 3]), 5, seg, pe, vals, None) == EARG
        assert re.search(r"\bclip 3\b", err()) and "-3" in err(), err()
        assert call(host_ctx, pa, pb, STRIDE, lens(LENS[:3] + [1024] + LENS[4:]), gr, 5, seg, pe, vals, None) == EARG
        assert re.search(r"\bclip 3\b", err()) and re.search(r"\b1024\b", err()), err()
        assert call(host_ctx, pa, pb, STRIDE, lens(LENS[:1] + [STRIDE + 1] + LENS[2:]), gr, 5, seg, pe, vals, None) == EARG
        assert re.search(r"\bclip 1\b", err()) and str(STRIDE + 1) in err() and "stride" in err(), err()
        assert call(host_ctx, pa, pb, STRIDE - 1, gl, gr, 5, seg, pe, vals, None) == EARG
        assert re.search(r"\bclip 0\b", err()) and str(STRIDE) in err(), err()
        assert call(host_ctx, pa, pb, STRIDE, lens([LENS[0], 7, LENS[2], 1024, LENS[4]]), rows([2, 1, 0, 2, 3]), 5, seg, pe, vals, None) == EARG
        assert re.search(r"\bclip 1\b", err()) and re.search(r"\b7 samples\b", err()), err()
    # more frame rows than a call, or one segment of it, takes
    assert call(host_ctx, pa, pb, 1 << 40, lens([1 << 40]), None, 1, 256, pe, vals, None) == EARG
    assert "too many" in err(), err()
    assert call(host_ctx, pa, pb, STRIDE, lens(LENS[:2]), rows([2 ** 31 - 1, 2 ** 31 - 1]), 2, 1, pe, vals, None) == EARG
    assert "too many" in err(), err()
    assert call(host_ctx, pa, pb, 1 << 36, lens([1 << 36, 1 << 36]), rows([8, 8]), 2, 1 << 30, pe, vals, None) == EARG
    assert "too many" in err(), err()
    # the estimate over the mixture or the clean signal: segmented or delegating
    for seg in (1, 3, 10, 256):
        assert call(host_ctx, pa, pb, STRIDE, gl, gr, 5, seg, pa, vals, None) == EARG
        assert "overlap" in err()
        assert call(host_ctx, pa, pb, STRIDE, gl, gr, 5, seg, pb, vals, None) == EARG
        assert "overlap" in err()
    # valid arguments, with and without row counts and an estimate, segmented or delegating: a host-only context cannot compute
    for seg in (1, 3, 10, 256):
        assert call(host_ctx, pa, pb, STRIDE, gl, gr, 5, seg, pe, vals, None) == ESTATE
        assert "host-only" in err()
        assert call(host_ctx, pa, pb, STRIDE, gl, None, 5, seg, None, vals, None) == ESTATE
    assert not a.any() and not b.any() and not e.any() and not any(vals)
    assert list(gl) == LENS and list(gr) == ROWS                 # the arrays are the caller's: read, not written


def test_python_methods_exist_and_check_first(native):
    import torch
    from speechseparation_amd import metrics
    from speechseparation_amd.bsrnn import BSRNN
    sig = inspect.signature(BSRNN.evaluate_long_ragged)
    assert list(sig.parameters) == ["self", "mix", "speech", "lengths", "clip_rows", "segment_frames", "return_estimate"]
    assert sig.parameters["clip_rows"].default is None and sig.parameters["segment_frames"].default == 256
    assert sig.parameters["return_estimate"].default is False
    sig = inspect.signature(BSRNN.evaluate_long)
    assert list(sig.parameters) == ["self", "mix", "speech", "segment_frames", "return_estimate"]
    assert sig.parameters["segment_frames"].default == 256 and sig.parameters["return_estimate"].default is False
    sig = inspect.signature(BSRNN.evaluate_many_long)
    assert list(sig.parameters) == ["self", "pairs", "segment_frames", "max_rows"]
    assert sig.parameters["segment_frames"].default == 256 and sig.parameters["max_rows"].default == 64
    sig = inspect.signature(metrics.evaluate_many_long)
    assert list(sig.parameters) == ["model", "pairs", "segment_frames", "max_rows"]
    assert sig.parameters["segment_frames"].default == 256 and sig.parameters["max_rows"].default == 64
    # the existing calls keep their signatures
    assert list(inspect.signature(BSRNN.evaluate_ragged).parameters) == ["self", "mix", "speech", "lengths", "clip_rows", "return_estimate"]
    assert list(inspect.signature(BSRNN.evaluate_many).parameters) == ["self", "pairs", "max_rows", "max_padding"]
    m = BSRNN()
    w = torch.zeros((3, 5000))
    pair = (torch.zeros(5000), torch.zeros(5000))
    # shape, length and segment errors, before any device is asked for (there is none here, and no context afterwards)
    for bad in (lambda: m.evaluate_long_ragged(torch.zeros(5000), torch.zeros(5000), [5000]),       # not [R, n_max]
                lambda: m.evaluate_long_ragged(w, torch.zeros((3, 4000)), [5000] * 3),              # mix and speech differ
                lambda: m.evaluate_long_ragged(w, "speech", [5000] * 3),
                lambda: m.evaluate_long_ragged(w, w, [5000, 5000]),                                 # two clips of one row for three rows
                lambda: m.evaluate_long_ragged(w, w, [5000, 4000], [2, 2]),                         # four rows for three
                lambda: m.evaluate_long_ragged(w, w, [5000, 4000], [3]),                            # one row count for two clips
                lambda: m.evaluate_long_ragged(w, w, [5000, 4000], [3, 0]),                         # a clip without rows
                lambda: m.evaluate_long_ragged(w, w, [5000, 1024], [2, 1]),                         # no reflect padding
                lambda: m.evaluate_long_ragged(w, w, [5000, 5001], [2, 1]),                         # longer than the row
                lambda: m.evaluate_long_ragged(w, w, [], []),
                lambda: m.evaluate_long_ragged(w, w, 5000),                                         # not a sequence
                lambda: m.evaluate_long_ragged(w, w, [5000], 3),
                lambda: m.evaluate_long_ragged(w, w, [5000], [3], 0),                               # no frames in a segment
                lambda: m.evaluate_long_ragged(w, w, [5000], [3], -2),
                lambda: m.evaluate_long_ragged(w, w, [5000], [3], "many"),
                lambda: m.evaluate_long_ragged(w, w, [5000], [3], segment_frames=None),
                lambda: m.evaluate_long(torch.zeros(5000), torch.zeros(5000)),                      # not [R, n]
                lambda: m.evaluate_long(w, torch.zeros((3, 4000))),
                lambda: m.evaluate_long(w, "speech"),
                lambda: m.evaluate_long(torch.zeros((2, 1024)), torch.zeros((2, 1024))),            # no reflect padding
                lambda: m.evaluate_long(w, w, 0),
                lambda: m.evaluate_long(w, w, segment_frames="many"),
                lambda: m.evaluate_many_long([(torch.zeros(5000), torch.zeros((1, 5000)))]),        # [n] against [ch, n]
                lambda: m.evaluate_many_long([(torch.zeros((2, 5000)), torch.zeros((1, 5000)))]),   # channel counts differ
                lambda: m.evaluate_many_long([(torch.zeros(5000), torch.zeros(1024))]),             # common length too short
                lambda: m.evaluate_many_long([pair, torch.zeros(5000)]),
                lambda: m.evaluate_many_long([(torch.zeros(5000), "speech")]),
                lambda: m.evaluate_many_long([pair], max_rows=0),
                lambda: m.evaluate_many_long([pair], segment_frames=0),
                lambda: m.evaluate_many_long([], segment_frames=0),
                lambda: m.evaluate_many_long([pair], "many"),
                lambda: metrics.evaluate_many_long(m, [(torch.zeros(5000), torch.zeros(100))]),
                lambda: metrics.evaluate_many_long(m, [pair], segment_frames=-1)):
        with pytest.raises(ValueError):
            bad()
    assert m.evaluate_many_long([]) == [] and metrics.evaluate_many_long(m, []) == []
    assert m._ctx is None and m.workspace_rows() == 0


def test_validate_has_the_segment_frames_option():
    src = open(os.path.join(REPO, "validate.py")).read()
    assert re.search(r'add_argument\("--segment-frames", type=int, default=0', src)
    assert re.search(r'add_argument\("--batch-rows", type=int, default=0', src)
    assert "evaluate_many_long" in src


# ------------------------------------------------------------------------------------------------ plan_host.h and metrics_host.h
def test_segment_coverage_and_sisdr_from_totals(tmp_path):
    exe = str(tmp_path / "evaluate_long_check")
    src = os.path.join(REPO, "tests", "cpp", "evaluate_long_check.cpp")
    text = open(src).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["metrics_host.h", "plan_host.h"]          # host headers only
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, src, "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "ok", out.stdout + out.stderr
