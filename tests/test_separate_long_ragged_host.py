"""CPU-side tests of the ragged long-form interface (bsrnn_separate_long_ragged, BSRNN.separate_long_ragged / separate_many_long,
spec.long_plan / long_buckets): the plan of plan_host.h against a brute-force restatement (through the small program
tests/cpp/ragged_long_plan_check.cpp) and spec.long_plan against that program, the bucketing, the declaration, the export and the
binding, argument checking on a host-only context, and the Python methods' shape errors.  No compute here;
tests/test_gpu_separate_long_ragged.py holds the arithmetic."""
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
LENS = [9293, 9216, 7167, 3077, 1025]          # the five rows of the GPU tests: 10 / 10 / 7 / 4 / 2 frames
NAME = "bsrnn_separate_long_ragged"


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


# ------------------------------------------------------------------------------------------------ the plan: plan_host.h and spec.long_plan
@pytest.fixture(scope="module")
def plan_cases(tmp_path_factory):
    """The small program's cases: it checks ragged_long_plan against the definition itself and prints what it got."""
    exe = str(tmp_path_factory.mktemp("plan") / "ragged_long_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "ragged_long_plan_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", [ln for ln in lines if ln.startswith("BAD")] or lines[-3:]
    cases = []
    for ln in lines[:-1]:
        head, rows, total = (part.split() for part in ln.split("|"))
        cases.append((int(head[0]), int(head[1]), [int(x) for x in head[2:]], [int(x) for x in rows], int(total[0])))
    return cases


def test_plan_arithmetic_cpp(plan_cases):
    assert len(plan_cases) > 300
    segs = {c[0] for c in plan_cases}
    assert 1 in segs and max(segs) > 10
    assert any(n % 1024 == 0 for c in plan_cases for n in c[2])                           # a length that is a multiple of 1024
    assert all(c[3] == sorted(c[3], reverse=True) for c in plan_cases)                    # the prefix never grows
    assert any(len(set(c[3])) > 2 for c in plan_cases)                                    # ... and does shrink, more than once


def test_long_plan_agrees_with_the_cpp_plan(plan_cases):
    for seg, stride, lens, rows, total in plan_cases:
        frames = [spec.n_frames(n) for n in lens]
        assert spec.long_plan(frames, seg) == (rows, total), (seg, lens)
        assert sum(frames) <= total <= len(frames) * max(frames)


def test_long_plan_literals():
    frames = [spec.n_frames(n) for n in LENS]
    assert frames == [10, 10, 7, 4, 2]
    assert spec.long_plan(frames, 3) == ([5, 4, 3, 2], 38)
    assert spec.long_plan(frames, 1) == ([5, 5, 4, 4, 3, 3, 3, 2, 2, 2], 33)
    assert spec.long_plan([10, 2, 7, 10, 4], 3) == ([5, 5, 4, 4], 46)                     # ended rows inside the prefix are paid for
    assert spec.long_plan(frames, 10) == ([5], 50) and spec.long_plan(frames, 999) == ([5], 50)
    assert spec.long_plan([7], 2) == ([1, 1, 1, 1], 7)
    for bad in (lambda: spec.long_plan([], 3), lambda: spec.long_plan([3, 0], 3), lambda: spec.long_plan([3], 0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ spec.long_buckets
def check_long_buckets(frames, rows, max_rows):
    buckets = spec.long_buckets(frames, rows, max_rows)
    assert sorted(i for b in buckets for i in b) == list(range(len(frames))), (frames, rows, buckets)      # a partition of the clips
    assert all(len(b) > 0 for b in buckets)
    for b in buckets:
        assert sum(rows[i] for i in b) <= max_rows or len(b) == 1, (frames, rows, max_rows, b)
    order = [i for b in buckets for i in b]
    assert order == sorted(range(len(frames)), key=lambda j: (-frames[j], j))             # longest first inside and across buckets
    assert spec.long_buckets(list(frames), list(rows), max_rows) == buckets               # deterministic
    return buckets


def test_long_buckets_random():
    rng = random.Random(20241)
    for _ in range(300):
        n = rng.randint(1, 40)
        frames = [rng.randint(2, 3000) for _ in range(n)]
        rows = [rng.choice((1, 1, 2, 2, 2, 6)) for _ in range(n)]
        check_long_buckets(frames, rows, rng.choice((1, 2, 4, 7, 64)))


def test_long_buckets_edges():
    assert check_long_buckets([], [], 64) == []
    assert check_long_buckets([10], [2], 64) == [[0]]
    assert check_long_buckets([7] * 5, [2] * 5, 4) == [[0, 1], [2, 3], [4]]
    # no padding cap: clips of very different lengths share a bucket (ragged_buckets at 25 % would split them)
    assert check_long_buckets([2048, 64, 700, 64], [2, 2, 2, 2], 64) == [[0, 2, 1, 3]]
    assert len(spec.ragged_buckets([2048, 64, 700, 64], [2, 2, 2, 2], 64, 0.25)) == 3
    # a clip wider than the cap is alone in its bucket; the others still obey the cap
    b = check_long_buckets([8, 9, 8, 8], [2, 6, 2, 2], 4)
    assert b == [[1], [0, 2], [3]]
    with pytest.raises(ValueError):
        spec.long_buckets([3, 4], [1], 64)
    with pytest.raises(ValueError):
        spec.long_buckets([3], [1], 0)
    with pytest.raises(ValueError):
        spec.long_buckets([3], [0], 4)


def test_spec_needs_no_torch():
    src = inspect.getsource(spec)
    assert "import torch" not in src and "import numpy" not in src


# ------------------------------------------------------------------------------------------------ the symbol
def test_header_declares_the_symbol():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % NAME, txt, flags=re.M)
    assert m and m.group(1).strip() == "int"
    types = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
    assert types == ["bsrnn_ctx*", "constfloat*", "int64_t", "constint64_t*", "float*", "int32_t", "int32_t", "void*"]
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)


def test_symbol_is_listed_bound_and_exported(native):
    assert NAME in native.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert NAME in set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_separate_long_ragged.argtypes == [vp, vp, i64, vp, vp, i32, i32, vp]
    assert native.lib.bsrnn_separate_long_ragged.restype == ctypes.c_int
    assert native.lib.bsrnn_abi_version() == 2
    # the counter of frame rows exists, the one behind it does not
    assert native.lib.bsrnn_debug_counter(4) >= 0 and native.lib.bsrnn_debug_counter(5) == -1


def test_argument_errors_without_a_device(native, host_ctx):
    fn = native.lib.bsrnn_separate_long_ragged
    stride = LENS[0]
    a, b = np.zeros((5, stride), np.float32), np.zeros((5, 9 * 1024), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)

    def lens(values):
        return (ctypes.c_int64 * len(values))(*values)

    def err():
        return native.lib.bsrnn_last_error().decode()
    good = lens(LENS)
    # each null argument, no rows, no frames per segment
    assert fn(None, pa, stride, good, pb, 5, 3, None) == EARG
    assert fn(host_ctx, None, stride, good, pb, 5, 3, None) == EARG
    assert fn(host_ctx, pa, stride, None, pb, 5, 3, None) == EARG
    assert fn(host_ctx, pa, stride, good, None, 5, 3, None) == EARG
    assert fn(host_ctx, pa, stride, good, pb, 0, 3, None) == EARG
    assert fn(host_ctx, pa, stride, good, pb, 5, 0, None) == EARG
    assert "seg_frames" in err(), err()
    assert fn(host_ctx, pa, stride, good, pb, 5, -4, None) == EARG
    # a row without reflect padding, a row longer than the stride: the text names the row and the value
    assert fn(host_ctx, pa, stride, lens(LENS[:3] + [1024] + LENS[4:]), pb, 5, 3, None) == EARG
    assert re.search(r"\brow 3\b", err()) and re.search(r"\b1024\b", err()), err()
    assert fn(host_ctx, pa, stride, lens(LENS[:2] + [stride + 1] + LENS[3:]), pb, 5, 3, None) == EARG
    assert re.search(r"\brow 2\b", err()) and str(stride + 1) in err() and "stride" in err(), err()
    assert fn(host_ctx, pa, stride - 1, good, pb, 5, 3, None) == EARG
    assert re.search(r"\brow 0\b", err()) and str(stride) in err(), err()
    # wave_out overlapping wave: the host-only context has the default range policy and cannot change it, so the refusal under either
    # policy is checked where a device context exists (tests/test_gpu_separate_long_ragged.py); here with segments and with one segment
    for seg in (3, 10, 400):
        assert fn(host_ctx, pa, stride, good, pa, 5, seg, None) == EARG
        assert "overlap" in err(), err()
    # valid arguments: a host-only context cannot compute, in segments or as the one ragged call
    for seg in (1, 3, 10, 400):
        assert fn(host_ctx, pa, stride, good, pb, 5, seg, None) == ESTATE
        assert "host-only" in err()
    assert not a.any() and not b.any()
    assert list(good) == LENS                                # the lengths are the caller's: read, not written


def test_python_methods_exist_and_check_shapes_first(native):
    import torch
    from speechseparation_amd.bsrnn import BSRNN
    sig = inspect.signature(BSRNN.separate_long_ragged)
    assert list(sig.parameters) == ["self", "waveform", "lengths", "segment_frames", "out"]
    assert sig.parameters["segment_frames"].default == 256 and sig.parameters["out"].default is None
    sig = inspect.signature(BSRNN.separate_many_long)
    assert list(sig.parameters) == ["self", "clips", "segment_frames", "max_rows"]
    assert sig.parameters["segment_frames"].default == 256 and sig.parameters["max_rows"].default == 64
    # separate_many keeps its signature
    assert list(inspect.signature(BSRNN.separate_many).parameters) == ["self", "clips", "max_rows", "max_padding"]
    m = BSRNN()
    w = torch.zeros((2, 5000))
    # shape and length errors, before any device is asked for (there is none here, and no context afterwards)
    for bad in (lambda: m.separate_long_ragged(torch.zeros(5000), [5000]),              # not [R, n_max]
                lambda: m.separate_long_ragged(w, [5000]),                              # one length for two rows
                lambda: m.separate_long_ragged(w, [5000, 1024]),                        # no reflect padding
                lambda: m.separate_long_ragged(w, [5000, 5001]),                        # longer than the row
                lambda: m.separate_long_ragged(w, 5000),                                # not a sequence
                lambda: m.separate_long_ragged(w, [5000, 4000], 0),                     # no frames per segment
                lambda: m.separate_long_ragged(w, [5000, 4000], "many"),
                lambda: m.separate_long_ragged(w, [5000, 4000], 3, out="no tensor"),
                lambda: m.separate_many_long([torch.zeros(5000), torch.zeros((1, 2, 5000))]),
                lambda: m.separate_many_long([torch.zeros(1024)]),
                lambda: m.separate_many_long([torch.zeros((2, 5000)), "clip"]),
                lambda: m.separate_many_long([torch.zeros(5000)], segment_frames=0),
                lambda: m.separate_many_long([torch.zeros(5000)], max_rows=0)):
        with pytest.raises(ValueError):
            bad()
    assert m.separate_many_long([]) == []
    assert m._ctx is None and m.workspace_rows() == 0
