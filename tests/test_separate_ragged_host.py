"""CPU-side tests of the ragged-batch interface (bsrnn_separate_ragged, BSRNN.separate_ragged / separate_many, spec.ragged_buckets):
the declaration, the export and the binding, argument checking on a host-only context, the Python methods' shape errors, the bucketing
and the shape arithmetic of plan_host.h (through the small program tests/cpp/ragged_shape_check.cpp).  No compute here;
tests/test_gpu_separate_ragged.py holds the arithmetic."""
import ctypes
import inspect
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from speechseparation_amd import spec

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
LENS = [9 * 1024 + 77, 3 * 1024 + 5, 4 * 1024, 7 * 1024 + 1023, 8 * 1024 + 1, 1025]


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
    m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+bsrnn_separate_ragged\s*\(([^)]*)\)\s*;", txt, flags=re.M)
    assert m and m.group(1).strip() == "int"
    types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
    assert types == ["bsrnn_ctx*", "constfloat*", "int64_t", "constint64_t*", "float*", "int32_t", "void*"]
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)


def test_symbol_is_listed_bound_and_exported(native):
    assert "bsrnn_separate_ragged" in native.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert "bsrnn_separate_ragged" in set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_separate_ragged.argtypes == [vp, vp, i64, vp, vp, i32, vp]
    assert native.lib.bsrnn_separate_ragged.restype == ctypes.c_int
    assert native.lib.bsrnn_abi_version() == 2


def test_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib
    stride = LENS[0]
    a, b = np.zeros((6, stride), np.float32), np.zeros((6, 9 * 1024), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)

    def lens(values):
        return (ctypes.c_int64 * len(values))(*values)

    def err():
        return lib.bsrnn_last_error().decode()
    good = lens(LENS)
    # each null argument, and no rows
    assert lib.bsrnn_separate_ragged(None, pa, stride, good, pb, 6, None) == EARG
    assert lib.bsrnn_separate_ragged(host_ctx, None, stride, good, pb, 6, None) == EARG
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride, None, pb, 6, None) == EARG
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride, good, None, 6, None) == EARG
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride, good, pb, 0, None) == EARG
    # a row without reflect padding, a row longer than the stride: the text names the row and the value
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride, lens(LENS[:4] + [1024] + LENS[5:]), pb, 6, None) == EARG
    assert re.search(r"\brow 4\b", err()) and re.search(r"\b1024\b", err()), err()
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride, lens(LENS[:2] + [stride + 1] + LENS[3:]), pb, 6, None) == EARG
    assert re.search(r"\brow 2\b", err()) and str(stride + 1) in err() and "stride" in err(), err()
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride - 1, good, pb, 6, None) == EARG
    assert re.search(r"\brow 0\b", err()) and str(stride) in err(), err()
    # valid arguments: a host-only context cannot compute
    assert lib.bsrnn_separate_ragged(host_ctx, pa, stride, good, pb, 6, None) == ESTATE
    assert "host-only" in err()
    assert not a.any() and not b.any()
    assert list(good) == LENS                                # the lengths are the caller's: read, not written


def test_python_methods_exist_and_check_shapes_first(native):
    import torch
    from speechseparation_amd.bsrnn import BSRNN
    sig = inspect.signature(BSRNN.separate_ragged)
    assert list(sig.parameters) == ["self", "waveform", "lengths", "out"] and sig.parameters["out"].default is None
    sig = inspect.signature(BSRNN.separate_many)
    assert list(sig.parameters) == ["self", "clips", "max_rows", "max_padding"]
    assert sig.parameters["max_rows"].default == 64 and sig.parameters["max_padding"].default == 0.25
    m = BSRNN()
    w = torch.zeros((2, 5000))
    # shape and length errors, before any device is asked for (there is none here, and no context afterwards)
    for bad in (lambda: m.separate_ragged(torch.zeros(5000), [5000]),              # not [R, n_max]
                lambda: m.separate_ragged(w, [5000]),                              # one length for two rows
                lambda: m.separate_ragged(w, [5000, 1024]),                        # no reflect padding
                lambda: m.separate_ragged(w, [5000, 5001]),                        # longer than the row
                lambda: m.separate_ragged(w, 5000),                                # not a sequence
                lambda: m.separate_ragged(w, [5000, 4000], out="no tensor"),
                lambda: m.separate_many([torch.zeros(5000), torch.zeros((1, 2, 5000))]),
                lambda: m.separate_many([torch.zeros(1024)]),
                lambda: m.separate_many([torch.zeros((2, 5000)), "clip"]),
                lambda: m.separate_many([torch.zeros(5000)], max_rows=0),
                lambda: m.separate_many([torch.zeros(5000)], max_padding=1.0)):
        with pytest.raises(ValueError):
            bad()
    assert m.separate_many([]) == []
    assert m._ctx is None and m.workspace_rows() == 0


# ------------------------------------------------------------------------------------------------ spec.ragged_buckets
def padding_share(frames, rows, bucket):
    return 1 - sum(rows[i] * frames[i] for i in bucket) / (sum(rows[i] for i in bucket) * max(frames[i] for i in bucket))


def check_buckets(frames, rows, max_rows, max_padding):
    buckets = spec.ragged_buckets(frames, rows, max_rows, max_padding)
    # a partition of the clips (a clip is one index: its channels stay together by construction of the interface, and its rows count whole)
    assert sorted(i for b in buckets for i in b) == list(range(len(frames))), (frames, rows, buckets)
    assert all(len(b) > 0 for b in buckets)
    for b in buckets:
        n_rows = sum(rows[i] for i in b)
        assert n_rows <= max_rows or len(b) == 1, (frames, rows, max_rows, b)
        assert padding_share(frames, rows, b) <= max_padding, (frames, rows, max_padding, b)
    assert spec.ragged_buckets(list(frames), list(rows), max_rows, max_padding) == buckets       # deterministic
    return buckets


def test_ragged_buckets_random():
    rng = random.Random(20240)
    for _ in range(300):
        n = rng.randint(1, 40)
        frames = [rng.randint(2, 130) for _ in range(n)]
        rows = [rng.choice((1, 1, 2, 2, 2, 6)) for _ in range(n)]
        check_buckets(frames, rows, rng.choice((1, 2, 4, 7, 64)), rng.choice((0.0, 0.05, 0.25, 0.5, 0.9)))


def test_ragged_buckets_edges():
    assert check_buckets([10], [2], 64, 0.25) == [[0]]                               # one clip
    assert check_buckets([], [], 64, 0.25) == []
    assert check_buckets([7] * 5, [2] * 5, 64, 0.25) == [[0, 1, 2, 3, 4]]            # all equal: one bucket, no padding ...
    assert check_buckets([7] * 5, [2] * 5, 4, 0.0) == [[0, 1], [2, 3], [4]]          # ... cut by the row cap alone
    # max_padding = 0: only clips of the same frame count share a bucket
    b = check_buckets([5, 9, 5, 9, 3], [1, 2, 1, 2, 1], 64, 0.0)
    assert b == [[1, 3], [0, 2], [4]]
    # a clip with more rows than max_rows gets a bucket of its own; the others still obey the cap
    b = check_buckets([8, 8, 8, 8], [2, 6, 2, 2], 4, 0.25)
    assert [1] in b and all(sum((2, 6, 2, 2)[i] for i in x) <= 4 for x in b if x != [1])
    # longest first, so a bucket's longest clip is its first; the default caps on the six lengths of the GPU tests
    frames = [1 + n // 1024 for n in LENS]
    b = check_buckets(frames, [1] * 6, 64, 0.25)
    assert b[0][0] == 0 and all(frames[x[0]] == max(frames[i] for i in x) for x in b)
    with pytest.raises(ValueError):
        spec.ragged_buckets([3, 4], [1], 64, 0.25)
    with pytest.raises(ValueError):
        spec.ragged_buckets([3], [1], 0, 0.25)


def test_ragged_buckets_needs_no_torch():
    src = inspect.getsource(spec)
    assert "import torch" not in src and "import numpy" not in src


# ------------------------------------------------------------------------------------------------ the shape arithmetic of plan_host.h
def test_ragged_shape_arithmetic(tmp_path):
    exe = str(tmp_path / "ragged_shape_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "ragged_shape_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
