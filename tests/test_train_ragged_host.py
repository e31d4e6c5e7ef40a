"""CPU-side tests of ragged training (bsrnn_stft_ragged, bsrnn_istft_ragged, bsrnn_istft_ragged_backward, bsrnn_train_loss_ragged and its
backward; train.stft_ragged / train_loss_ragged / train_backward_many / train_step_many): the declarations, the exports and the bindings,
argument checking on a host-only context, the clip table of train_ragged_host.h (through the small program
tests/cpp/train_ragged_check.cpp, built with the address and undefined-behaviour sanitizers) and train_backward_many's bucketing and
packing up to the first native call.  No compute here; tests/test_gpu_train_ragged.py holds the arithmetic."""
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
NEW = ["bsrnn_stft_ragged", "bsrnn_istft_ragged", "bsrnn_istft_ragged_backward", "bsrnn_train_loss_ragged", "bsrnn_train_loss_ragged_backward"]
LENS = [5 * 1024 + 300, 3 * 1024 + 77, 1025, 6 * 1024]      # T = 6, 4, 2, 7
STRIDE = 6 * 1024 + 3


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


def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {
        "bsrnn_stft_ragged": ["bsrnn_ctx*", "constfloat*", "int64_t", "constint64_t*", "float*", "int32_t", "void*"],
        "bsrnn_istft_ragged": ["bsrnn_ctx*", "constfloat*", "constint64_t*", "float*", "int32_t", "void*"],
        "bsrnn_istft_ragged_backward": ["bsrnn_ctx*", "constfloat*", "constint64_t*", "float*", "int32_t", "void*"],
        "bsrnn_train_loss_ragged": ["bsrnn_ctx*", "constfloat*", "constfloat*", "constfloat*", "constfloat*", "int64_t", "constint64_t*",
                                    "constint32_t*", "int32_t", "double*", "double*", "void*"],
        "bsrnn_train_loss_ragged_backward": ["bsrnn_ctx*", "constfloat*", "constfloat*", "constfloat*", "constfloat*", "int64_t", "constint64_t*",
                                             "constint32_t*", "int32_t", "constdouble*", "constfloat*", "float*", "float*", "void*"],
    }
    for name, types in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, txt, flags=re.M)
        assert m and m.group(1).strip() == "int", name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, (name, got)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", txt)
    assert re.search(r"#define\s+BSRNN_N_TRAIN_VALUES\s+5\b", txt)
    for i, name in enumerate(("LOSS", "L1_TIME", "L1_RE", "L1_IM", "SDR")):
        assert re.search(r"#define\s+BSRNN_TV_%s\s+%d\b" % (name, i), txt)


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    args = {
        "bsrnn_stft_ragged": [vp, vp, i64, vp, vp, i32, vp],
        "bsrnn_istft_ragged": [vp, vp, vp, vp, i32, vp],
        "bsrnn_istft_ragged_backward": [vp, vp, vp, vp, i32, vp],
        "bsrnn_train_loss_ragged": [vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp],
        "bsrnn_train_loss_ragged_backward": [vp, vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, vp],
    }
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
        assert getattr(native.lib, name).argtypes == args[name] and getattr(native.lib, name).restype == ctypes.c_int, name
    assert native.TRAIN_VALUE_NAMES == ("loss", "l1_time", "l1_re", "l1_im", "sdr")
    assert native.lib.bsrnn_abi_version() == 2


def _lens(values):
    return (ctypes.c_int64 * len(values))(*values)


def _rows(values):
    return (ctypes.c_int32 * len(values))(*values)


def test_dsp_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib
    a = np.zeros((4, STRIDE), np.float32)
    b = np.zeros((4, 2050 * 7), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)

    def err():
        return lib.bsrnn_last_error().decode()
    good = _lens(LENS)
    calls = {
        "bsrnn_stft_ragged": lambda ctx, src, lens, dst, R: lib.bsrnn_stft_ragged(ctx, src, STRIDE, lens, dst, R, None),
        "bsrnn_istft_ragged": lambda ctx, src, lens, dst, R: lib.bsrnn_istft_ragged(ctx, src, lens, dst, R, None),
        "bsrnn_istft_ragged_backward": lambda ctx, src, lens, dst, R: lib.bsrnn_istft_ragged_backward(ctx, src, lens, dst, R, None),
    }
    for name, call in calls.items():
        # each null argument, and no rows
        assert call(None, pa, good, pb, 4) == EARG, name
        assert call(host_ctx, None, good, pb, 4) == EARG, name
        assert call(host_ctx, pa, None, pb, 4) == EARG, name
        assert call(host_ctx, pa, good, None, 4) == EARG, name
        assert call(host_ctx, pa, good, pb, 0) == EARG, name
        # a row without reflect padding: the text names the call, the row and the value
        assert call(host_ctx, pa, _lens(LENS[:2] + [1024] + LENS[3:]), pb, 4) == EARG, name
        assert name + ":" in err() and re.search(r"\brow 2\b", err()) and re.search(r"\b1024\b", err()), err()
        assert call(host_ctx, pa, _lens([7] + LENS[1:]), pb, 4) == EARG, name
        assert re.search(r"\brow 0\b", err()) and re.search(r"\b7 samples\b", err()), err()
        # more frame rows than one ragged call takes (a length the analysis's stride would refuse first)
        if name != "bsrnn_stft_ragged":
            assert call(host_ctx, pa, _lens([1 << 40]), pb, 1) == EARG, name
            assert "too many" in err(), err()
        # valid arguments: a host-only context cannot compute
        assert call(host_ctx, pa, good, pb, 4) == ESTATE, name
        assert "host-only" in err(), err()
    # the analysis alone has a row stride: a row longer than it, naming the row and the value
    assert lib.bsrnn_stft_ragged(host_ctx, pa, STRIDE, _lens(LENS[:1] + [STRIDE + 1] + LENS[2:]), pb, 4, None) == EARG
    assert re.search(r"\brow 1\b", err()) and str(STRIDE + 1) in err() and "stride" in err(), err()
    assert lib.bsrnn_stft_ragged(host_ctx, pa, 6 * 1024 - 1, good, pb, 4, None) == EARG
    assert re.search(r"\brow 3\b", err()) and str(6 * 1024) in err(), err()
    assert lib.bsrnn_stft_ragged(host_ctx, pa, 1 << 40, _lens([1 << 40]), pb, 1, None) == EARG
    assert "too many" in err(), err()
    # a length equal to the stride is fine
    assert lib.bsrnn_stft_ragged(host_ctx, pa, 6 * 1024, good, pb, 4, None) == ESTATE
    assert not a.any() and not b.any() and list(good) == LENS        # the lengths are the caller's: read, not written


def test_loss_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib
    R, clip_lens, clip_rows = 4, [LENS[0], LENS[1], LENS[2]], [2, 1, 1]
    y, s = np.zeros((R, 2050 * 6), np.float32), np.zeros((R, 2050 * 6), np.float32)
    xt, sp = np.zeros((R, 5 * 1024), np.float32), np.zeros((R, STRIDE), np.float32)
    dy, dx = np.zeros_like(y), np.zeros_like(xt)
    vals, sums, g = np.zeros((3, 5), np.float64), np.zeros((R, 2), np.float64), np.zeros((3, 2), np.float32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)       # noqa: E731

    def err():
        return lib.bsrnn_last_error().decode()

    def fwd(ctx=host_ctx, t=(y, s, xt, sp), stride=STRIDE, lens=clip_lens, rows=clip_rows, n=3, out=(vals, sums)):
        return lib.bsrnn_train_loss_ragged(ctx, *[None if x is None else p(x) for x in t], stride, None if lens is None else _lens(lens),
                                           None if rows is None else _rows(rows), n, *[None if x is None else p(x) for x in out], None)

    def bwd(ctx=host_ctx, t=(y, s, xt, sp), stride=STRIDE, lens=clip_lens, rows=clip_rows, n=3, out=(sums, g, dy, dx)):
        return lib.bsrnn_train_loss_ragged_backward(ctx, *[None if x is None else p(x) for x in t], stride, None if lens is None else _lens(lens),
                                                    None if rows is None else _rows(rows), n, *[None if x is None else p(x) for x in out], None)
    for name, call, outs in (("bsrnn_train_loss_ragged", fwd, (vals, sums)), ("bsrnn_train_loss_ragged_backward", bwd, (sums, g, dy, dx))):
        assert call(ctx=None) == EARG
        for i in range(4):                                   # each null tensor
            assert call(t=tuple(None if j == i else x for j, x in enumerate((y, s, xt, sp)))) == EARG, (name, i)
        for i in range(len(outs)):
            assert call(out=tuple(None if j == i else x for j, x in enumerate(outs))) == EARG, (name, i)
        assert call(lens=None) == EARG
        assert call(n=0) == EARG and call(n=-1) == EARG
        # a clip without rows, a clip without reflect padding, a clip longer than the stride: the text names the call, the clip and the value
        assert call(rows=[2, 0, 1]) == EARG
        assert name + ":" in err() and re.search(r"\bclip 1\b", err()) and re.search(r"\b0 rows\b", err()), err()
        assert call(rows=[2, 1, -3]) == EARG
        assert re.search(r"\bclip 2\b", err()) and "-3" in err(), err()
        assert call(lens=[LENS[0], 1024, LENS[2]]) == EARG
        assert re.search(r"\bclip 1\b", err()) and re.search(r"\b1024\b", err()), err()
        assert call(lens=[LENS[0], STRIDE + 1, LENS[2]]) == EARG
        assert re.search(r"\bclip 1\b", err()) and str(STRIDE + 1) in err() and "stride" in err(), err()
        assert call(stride=LENS[0] - 1) == EARG
        assert re.search(r"\bclip 0\b", err()) and str(LENS[0]) in err(), err()
        # the first offending clip is the one reported
        assert call(lens=[LENS[0], 7, 1024], rows=[2, 1, 0]) == EARG
        assert re.search(r"\bclip 1\b", err()) and re.search(r"\b7 samples\b", err()), err()
        # more frame rows than one ragged call takes
        assert call(stride=1 << 40, lens=[1 << 40], rows=None, n=1) == EARG
        assert "too many" in err(), err()
        assert call(lens=clip_lens[:2], rows=[2 ** 31 - 1, 2 ** 31 - 1], n=2) == EARG
        assert "too many" in err(), err()
        # valid arguments, with and without row counts: a host-only context cannot compute
        assert call() == ESTATE
        assert "host-only" in err(), err()
        assert call(rows=None) == ESTATE
    assert not any(x.any() for x in (y, s, xt, sp, dy, dx, vals, sums, g))


# ------------------------------------------------------------------------------------------------ train_ragged_host.h
def test_clip_table_arithmetic(tmp_path):
    exe = str(tmp_path / "train_ragged_check")
    src = os.path.join(REPO, "tests", "cpp", "train_ragged_check.cpp")
    text = open(src).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["train_ragged_host.h"]                     # host headers only
    header = open(os.path.join(CSRC, "train_ragged_host.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', header) == ["plan_host.h"] and "hip" not in header.lower().replace("api.hip", "")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, src, "-o", exe], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ the Python layer, without a device
def test_python_functions_exist_and_check_shapes_first(native):
    import torch
    from speechseparation_amd import train
    from speechseparation_amd.bsrnn import BSRNN
    sig = inspect.signature(train.train_loss_ragged)
    assert list(sig.parameters) == ["model", "mix", "speech", "lengths", "clip_rows"] and sig.parameters["clip_rows"].default is None
    sig = inspect.signature(train.train_backward_many)
    assert list(sig.parameters) == ["model", "pairs", "loss_sdr", "max_rows", "max_padding"]
    assert sig.parameters["loss_sdr"].default is False and sig.parameters["max_rows"].default == 64 and sig.parameters["max_padding"].default == 0.25
    sig = inspect.signature(train.train_step_many)
    assert list(sig.parameters)[:4] == ["model", "optimizer", "pairs", "group"] and sig.parameters["group"].default is None
    assert list(inspect.signature(train.stft_ragged).parameters) == ["wave", "lengths"]
    assert issubclass(train.IstftRaggedFunction, torch.autograd.Function) and issubclass(train.TriLossRaggedFunction, torch.autograd.Function)
    m = BSRNN()
    w = torch.zeros((3, 5000))
    z = torch.zeros(5000)
    for bad in (lambda: train.train_loss_ragged(m, z, z, [5000]),                                 # not [R, n_max]
                lambda: train.train_loss_ragged(m, w, torch.zeros((3, 4000)), [5000] * 3),        # mix and speech differ
                lambda: train.train_loss_ragged(m, w, "speech", [5000] * 3),
                lambda: train.train_loss_ragged(m, w, w, [5000, 5000]),                           # two clips of one row for three rows
                lambda: train.train_loss_ragged(m, w, w, [5000, 4000], [2, 2]),                   # four rows for three
                lambda: train.train_loss_ragged(m, w, w, [5000, 4000], [3]),
                lambda: train.train_loss_ragged(m, w, w, [5000, 4000], [3, 0]),                   # a clip without rows
                lambda: train.train_loss_ragged(m, w, w, [5000, 1024], [2, 1]),                   # no reflect padding
                lambda: train.train_loss_ragged(m, w, w, [5000, 5001], [2, 1]),                   # longer than the row
                lambda: train.train_loss_ragged(m, w, w, [], []),
                lambda: train.train_loss_ragged(m, w, w, 5000),                                   # not a sequence
                lambda: train.train_loss_ragged(m, w, w, [5000, 4000], [2, 1]),                   # valid shapes, but not on the GPU
                lambda: train.stft_ragged(z, [5000]),
                lambda: train.stft_ragged(w, [5000, 5000]),
                lambda: train.stft_ragged(w, [5000, 5000, 1024]),
                lambda: train.stft_ragged(w, [5000, 5000, 4000]),                                 # valid shapes, but not on the GPU
                lambda: train.train_backward_many(m, [(z, torch.zeros((1, 5000)))]),              # [n] against [ch, n]
                lambda: train.train_backward_many(m, [(torch.zeros((2, 5000)), torch.zeros((1, 5000)))]),
                lambda: train.train_backward_many(m, [(z, torch.zeros(1024))]),                   # common length too short
                lambda: train.train_backward_many(m, [(z, z), z]),
                lambda: train.train_backward_many(m, [(z, "speech")]),
                lambda: train.train_backward_many(m, [(torch.zeros((1, 2, 5000)), torch.zeros((1, 2, 5000)))]),
                lambda: train.train_backward_many(m, [(z, z)], max_rows=0),
                lambda: train.train_backward_many(m, [(z, z)], max_padding=1.0),
                lambda: train.train_backward_many(m, [(z, z)])):                                  # valid pairs, but nothing is on the GPU
        with pytest.raises(ValueError):
            bad()
    assert train.train_backward_many(m, []) == []
    assert all(p.grad is None for p in m.parameters())


def test_train_backward_many_buckets_and_packs(native, monkeypatch):
    """The bucketing and the packing on CPU tensors, up to the first native call: train_loss_ragged is replaced by a recorder."""
    import torch
    from speechseparation_amd import train
    from speechseparation_amd.bsrnn import BSRNN
    g = torch.Generator().manual_seed(5)
    ns = [5 * 1024 + 300, 1025, 5 * 1024 + 900, 3 * 1024 + 77, 1500]
    pairs = [(torch.randn((2, n + 11 * i), generator=g), torch.randn((2, n), generator=g)) for i, n in enumerate(ns)]
    pairs[3] = (pairs[3][0][0], pairs[3][1][0])                    # a mono pair [n]
    chans = [2, 2, 2, 1, 2]
    leaf = torch.zeros((), requires_grad=True)
    calls = []

    def recorder(model, mix, speech, lengths, clip_rows=None):
        calls.append((mix.clone(), speech.clone(), list(lengths), list(clip_rows)))
        k = len(calls)
        base = torch.tensor([100.0 * k + c for c in range(len(lengths))])
        return base + leaf, -base + 2 * leaf, None
    monkeypatch.setattr(train, "train_loss_ragged", recorder)
    m = BSRNN()
    out = train.train_backward_many(m, pairs, max_rows=4, max_padding=0.25)
    frames = [1 + n // 1024 for n in ns]
    buckets = spec.ragged_buckets(frames, chans, 4, 0.25)
    assert len(buckets) >= 2 and len(calls) == len(buckets)
    assert float(leaf.grad) == len(pairs)                          # one backward of losses.sum() per bucket, accumulated
    for k, (bucket, (mix, speech, lengths, clip_rows)) in enumerate(zip(buckets, calls), 1):
        assert lengths == [ns[i] for i in bucket] and clip_rows == [chans[i] for i in bucket]
        assert tuple(mix.shape) == tuple(speech.shape) == (sum(clip_rows), max(lengths))
        assert mix.dtype == torch.float32 and mix.is_contiguous() and speech.is_contiguous()
        r0 = 0
        for c, i in enumerate(bucket):
            ch, n = chans[i], ns[i]
            assert torch.equal(mix[r0:r0 + ch, :n], pairs[i][0].reshape(ch, -1)[:, :n])        # cut to the pair's common length
            assert torch.equal(speech[r0:r0 + ch, :n], pairs[i][1].reshape(ch, -1)[:, :n])
            assert not mix[r0:r0 + ch, n:].any() and not speech[r0:r0 + ch, n:].any()          # zeros behind a row's samples
            assert out[i] == (100.0 * k + c, -(100.0 * k + c))                                  # per pair, in input order
            r0 += ch
    # -sdr as the objective: d(-sdrs.sum()) / d leaf = -2 per clip
    leaf.grad = None
    calls.clear()
    train.train_backward_many(m, pairs, loss_sdr=True, max_rows=4)
    assert float(leaf.grad) == -2.0 * len(pairs)


def test_entry_point_has_the_ragged_flag():
    src = open(os.path.join(REPO, "train.py")).read()
    assert re.search(r'add_argument\("--ragged", action="store_true"', src)
    assert "train_step_many" in src
