"""GPU: the streaming FIR convolution (augment.FirStream -> bsrnn_fir_stream_*).

Under the SAME alignment the promise is an equality: the concatenated output of a row, flush included, is FirBank.convolve of the
concatenated input, bit for bit, for every way of cutting the input into calls - so these tests compare with the one-shot call, which
tests/test_gpu_convolve.py holds to the float64 definition.  Under the CAUSAL alignment there is no one-shot form: the result is held to
the project's DSP criterion (e <= 3 * e_f32 + 2^-24 * max|ref64|, per row and per block) against float64 numpy.convolve, with e_f32 from
the float32 model of the stream on the CPU (convolve_stream_reference.StreamModel) - never the kernel's own.

The shapes are convolve_reference.CASES, the smallest at which the kernel can go wrong: n = 1 (a), a filter longer than the row, everything
from the flush (h), an odd shift and unaligned stores (f), 44 partitions and 22 flush blocks (j), and a ring of three slots that wraps four
times."""
import ctypes

import numpy as np
import pytest
import torch

import convolve_reference as cr
import convolve_stream_reference as sr

pytestmark = pytest.mark.gpu
EARG = 1
B = 1024
NAMES = [c[0] for c in cr.CASES]
LENS = [c[2] for c in cr.CASES]
SENTINEL = 777.0
CUTS = ("once", "hops", "ragged")


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


@pytest.fixture(scope="module")
def bank(model):
    """One filter per case, in the table's order."""
    from speechseparation_amd.augment import FirBank
    return FirBank(model, [cr.case(name)[1] for name in NAMES])


@pytest.fixture(scope="module")
def oneshot(bank):
    """FirBank.convolve of the ten cases: what every stream below has to reproduce.  A list of tensors, computed once."""
    n_max = max(LENS)
    buf = torch.zeros((len(LENS), n_max), device="cuda")
    for r, name in enumerate(NAMES):
        buf[r, :LENS[r]] = torch.from_numpy(cr.case(name)[0].copy())
    res = bank.convolve(buf, LENS, list(range(len(LENS))))
    torch.cuda.synchronize()
    return [res[r, :n].clone() for r, n in enumerate(LENS)]


def row_cuts(n, kind, seed):
    return sr.cuttings(n, seed)[kind]


def call_counts(cuts):
    """Per-row lists of counts -> the calls: call c gives row r its c-th count, 0 once the row has none left."""
    return [[c[i] if i < len(c) else 0 for c in cuts] for i in range(max(len(c) for c in cuts))]


def process(st, xs, at, counts):
    """One process call that gives row r the next counts[r] samples of xs[r]: rows 3 floats further apart than the call needs, a value
    behind every count that must not be read, a sentinel behind every count that must not be written; the counts are ready()'s."""
    C, n = st.C, max(counts)
    wave = torch.full((C, n + 3), 5.0)
    for r in range(C):
        wave[r, :counts[r]] = torch.from_numpy(xs[r][at[r]:at[r] + counts[r]].copy())
    wave = wave.cuda()
    before = wave.clone()
    want = [st.ready(r, counts[r]) for r in range(C)]
    out = torch.full((C, max(want) + 3), SENTINEL, device="cuda")
    view = out[:, :max(want)]
    res, got = st.process(wave[:, :n], counts, out=view)
    assert res is view and got == want, (got, want)
    assert torch.equal(wave, before)                                         # the input is unchanged
    for r in range(C):
        assert bool((out[r, want[r]:] == SENTINEL).all()), r                 # nothing behind a row's count is written
        at[r] += counts[r]
    return [out[r, :want[r]].clone() for r in range(C)]


def flush(st, rows, owed):
    C = st.C
    out = torch.full((C, max(owed) + 3), SENTINEL, device="cuda")
    view = out[:, :max(owed)]
    res, got = st.flush(rows, out=view)
    assert res is view and got == owed, (got, owed)
    for r in range(C):
        assert bool((out[r, owed[r]:] == SENTINEL).all()), r
    return [out[r, :owed[r]].clone() for r in range(C)]


def owed_of(st, bank, r, n):
    f = st.filter_of(r)
    return 0 if f < 0 else n - sr.emitted(n, sr.shift_of(bank.taps(f), sr.CAUSAL if st.causal else sr.SAME))


def run(st, bank, xs, cuts):
    """xs[r] fed to row r in cuts[r], then every row flushed: the concatenated output per row."""
    C = st.C
    at, parts = [0] * C, [[] for _ in range(C)]
    for counts in call_counts(cuts):
        for r, p in enumerate(process(st, xs, at, counts)):
            parts[r].append(p)
    assert at == [x.shape[0] for x in xs]
    for r, p in enumerate(flush(st, None, [owed_of(st, bank, r, at[r]) for r in range(C)])):
        parts[r].append(p)
    return [torch.cat(p) for p in parts]


_ten = {}


def ten_rows(bank, kind):
    """The ten cases as the ten rows of one stream (max_taps = 44101, SAME), fed in the cutting `kind`; computed once per cutting."""
    if kind not in _ten:
        from speechseparation_amd.augment import FirStream
        st = FirStream(bank, len(NAMES), max_taps=44101)
        for r in range(len(NAMES)):
            st.assign([r], r)
        xs = [cr.case(name)[0] for name in NAMES]
        _ten[kind] = run(st, bank, xs, [row_cuts(LENS[r], kind, 50 + r) for r in range(len(NAMES))])      # every row draws on its own
    return _ten[kind]


@pytest.mark.parametrize("kind", CUTS)
def test_ten_cases_equal_the_one_shot(bank, oneshot, kind):
    got = ten_rows(bank, kind)
    for r, name in enumerate(NAMES):
        assert got[r].shape == oneshot[r].shape and torch.equal(got[r], oneshot[r]), (kind, name)


def test_the_ragged_cutting_mixes_held_partial_and_several_blocks():
    calls = call_counts([row_cuts(LENS[r], "ragged", 50 + r) for r in range(len(NAMES))])
    flat = [c for counts in calls for c in counts]
    assert 0 in flat and 1 in flat and 3000 in flat and any(0 in c and 3000 in c for c in calls)


def test_ring_wrap_at_the_smallest_depth(bank, model):
    """2049 taps: P = 3.  Twelve hops wrap a ring of three slots four times; one hop per call, five per call (two blocks of the call
    overwrite slots the call itself still reads from), and the same filter in a ring of 44 slots."""
    from speechseparation_amd.augment import FirStream
    g = NAMES.index("g")
    x = cr.signal(12 * B, 77)
    ref = bank.convolve(torch.from_numpy(x.copy()).cuda()[None, :], None, [g])[0]
    for max_taps, cuts in ((2049, [B] * 12), (2049, [5 * B, 5 * B, 2 * B]), (44101, [5 * B, 5 * B, 2 * B])):
        st = FirStream(bank, 1, max_taps=max_taps)
        st.assign([0], g)
        got = run(st, bank, [x], [cuts])[0]
        assert torch.equal(got, ref), (max_taps, cuts)


def test_a_row_equals_the_row_alone_and_bypass_is_the_input(bank, oneshot):
    from speechseparation_amd.augment import FirStream
    ten = ten_rows(bank, "ragged")
    for name in ("f", "i"):
        r = NAMES.index(name)
        st = FirStream(bank, 1, max_taps=44101)
        st.assign([0], r)
        alone = run(st, bank, [cr.case(name)[0]], [row_cuts(LENS[r], "ragged", 50 + r)])[0]
        assert torch.equal(alone, ten[r]), name
    # a bypass row between two filtered ones: its samples come back in the same call, its flush gives nothing
    st = FirStream(bank, 3, max_taps=2049)
    st.assign([0], NAMES.index("g"))
    st.assign([2], NAMES.index("d"))
    assert [st.filter_of(r) for r in range(3)] == [NAMES.index("g"), -1, NAMES.index("d")]
    xs = [cr.signal(3000, 31), cr.signal(2500, 32), cr.signal(3000, 33)]
    cuts = [[1000, 2000], [1, 1023, 0, 1476], [3000]]
    assert [st.ready(1, n) for n in (0, 1, 1023, 5000)] == [0, 1, 1023, 5000]
    got = run(st, bank, xs, cuts)
    assert torch.equal(got[1].cpu(), torch.from_numpy(xs[1].copy()))
    for r, name in ((0, "g"), (2, "d")):
        ref = bank.convolve(torch.from_numpy(xs[r].copy()).cuda()[None, :], None, [NAMES.index(name)])[0]
        assert torch.equal(got[r], ref), name


@pytest.mark.parametrize("how", ["assign", "reset"])
def test_assign_and_reset_in_the_middle_of_a_stream(bank, how):
    """Row 1 is moved (assign) or restarted (reset) after 1500 samples, with a block and a half in its ring, tail and FIFO: it continues as
    a fresh stream would, and rows 0 and 2 have the bits of an undisturbed run."""
    from speechseparation_amd.augment import FirStream
    fg, ff, fd, fe = (NAMES.index(c) for c in "gfde")
    st = FirStream(bank, 3, max_taps=2049)
    for r, f in enumerate((fg, ff, fd)):
        st.assign([r], f)
    xs = [cr.signal(4000, 41), cr.signal(1500, 42), cr.signal(4000, 43)]
    at, parts = [0, 0, 0], [[], [], []]
    for r, p in enumerate(process(st, xs, at, [1500, 1500, 1500])):
        parts[r].append(p)
    if how == "assign":
        st.assign([1], fe)
    else:
        st.reset([1])
    new_f = fe if how == "assign" else ff
    assert st.filter_of(1) == new_f and st.ready(1, B) == B - bank.taps(new_f) // 2
    fresh = cr.signal(2600, 44)
    xs[1], at[1], parts[1] = fresh, 0, []
    for counts in ([500, 500, 2500], [2000, 2100, 0]):
        for r, p in enumerate(process(st, xs, at, counts)):
            parts[r].append(p)
    for r, p in enumerate(flush(st, None, [owed_of(st, bank, r, at[r]) for r in range(3)])):
        parts[r].append(p)
    for r, f in enumerate((fg, new_f, fd)):
        ref = bank.convolve(torch.from_numpy(xs[r].copy()).cuda()[None, :], None, [f])[0]
        assert torch.equal(torch.cat(parts[r]), ref), (how, r)


def test_causal_alignment(bank):
    """y[m] = (x * g)[m]: cases b, f, i and j against float64 numpy.convolve, e_f32 from the CPU model fed in the same cutting."""
    from speechseparation_amd.augment import FirStream
    names = ["b", "f", "i", "j"]
    st = FirStream(bank, len(names), max_taps=44101, causal=True)
    for r, name in enumerate(names):
        st.assign([r], NAMES.index(name))
    xs = [cr.case(name)[0] for name in names]
    cuts = [row_cuts(x.shape[0], "ragged", 60 + r) for r, x in enumerate(xs)]
    assert [st.ready(r, n) for r, n in ((0, 1023), (1, 1024), (2, 2500))] == [0, 1024, 2048]      # latency under one hop
    got = run(st, bank, xs, cuts)
    for r, name in enumerate(names):
        x, h = cr.case(name)[:2]
        r64 = sr.causal_refs(x, h)[1]
        m32 = sr.StreamModel(h, sr.CAUSAL).run(x, cuts[r])
        assert got[r].shape[0] == x.shape[0]
        cr.hold_row("case %s, causal" % name, got[r].cpu().numpy(), m32, r64)


def test_no_ops_and_no_allocation(bank, oneshot):
    from speechseparation_amd import _native
    from speechseparation_amd.augment import FirStream
    f = NAMES.index("f")
    st = FirStream(bank, 2, max_taps=2049)
    st.assign([0, 1], f)
    x = cr.case("f")[0]
    counter = _native.lib.bsrnn_debug_counter(0)
    at, parts = [0, 0], []
    parts.append(process(st, [x, x], at, [1500, 0])[0])                      # row 1 takes nothing, ever
    assert process(st, [x, x], at, [0, 0]) [0].shape[0] == 0                 # a call with all counts 0 leaves all state as it was
    parts.append(process(st, [x, x], at, [1500, 0])[0])
    res = flush(st, [1], [0, 0])                                             # a row that took nothing: 0, and nothing is written
    assert res[0].shape[0] == 0 and res[1].shape[0] == 0
    parts.append(flush(st, [0], [owed_of(st, bank, 0, 3000), 0])[0])         # ... and row 0 was not touched by it
    torch.cuda.synchronize()
    assert _native.lib.bsrnn_debug_counter(0) == counter                     # nothing was allocated by process and flush
    assert torch.equal(torch.cat(parts), oneshot[f])


def test_refusals_and_the_next_call(bank, oneshot):
    """Every refusal returns BSRNN_EARG with its sentence before any device work, and the stream goes on to the first run's bits."""
    from speechseparation_amd import _native
    from speechseparation_amd.augment import FirStream
    lib = _native.lib
    f = NAMES.index("f")
    st = FirStream(bank, 2, max_taps=2049)
    st.assign([0, 1], f)
    x = cr.case("f")[0]
    at, parts = [0, 0], []
    parts.append(process(st, [x, x], at, [1100, 1100])[0])
    a = torch.zeros((2, 2000), device="cuda")
    b = torch.full((2, 2000), SENTINEL, device="cuda")
    pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
    i64s, i32s = (lambda *v: (ctypes.c_int64 * len(v))(*v)), (lambda *v: (ctypes.c_int32 * len(v))(*v))
    n_out = i64s(-7, -7)
    good = [st._h, pa, 2000, i64s(1000, 1000), pb, 2000, n_out, None]
    names = ["s", "in", "in_stride", "n_in", "out", "out_stride", "n_out", "stream"]

    def refused(sentence, **change):
        args = [change.get(k, v) for k, v in zip(names, good)]
        assert lib.bsrnn_fir_stream_process(*args) == EARG, sentence
        assert sentence in lib.bsrnn_last_error().decode(), lib.bsrnn_last_error().decode()
    refused("null FIR stream", s=None)
    refused("sample counts", n_in=None)
    refused("nowhere to report", n_out=None)
    refused("input block", **{"in": None})
    refused("output block", out=None)
    refused("n_in_host[1] = -1", n_in=i64s(1000, -1))
    refused("n_in_host[0] = %d" % ((1 << 30) + 1), n_in=i64s((1 << 30) + 1, 0), in_stride=1 << 31, out_stride=1 << 31)
    refused("in_stride = 999", in_stride=999)
    refused("out_stride = 1023", out_stride=1023)                            # 1100 + 1000 = 2100 taken: two blocks less the first call's, 1024 per row
    refused("overlap", out=pa)
    refused("overlap", out=ctypes.c_void_p(a.data_ptr() + 4 * 2999))         # the last sample the rows of the input span
    assert lib.bsrnn_fir_stream_flush_rows(st._h, i32s(0, 0), 2, pb, 2000, n_out, None) == EARG and "listed twice" in lib.bsrnn_last_error().decode()
    assert lib.bsrnn_fir_stream_flush_rows(st._h, i32s(2), 1, pb, 2000, n_out, None) == EARG and "row 2" in lib.bsrnn_last_error().decode()
    assert lib.bsrnn_fir_stream_flush_rows(st._h, i32s(0), 1, pb, 100, n_out, None) == EARG and "out_stride = 100" in lib.bsrnn_last_error().decode()
    assert lib.bsrnn_fir_stream_assign(st._h, i32s(0), 1, NAMES.index("j")) == EARG and "44101 taps" in lib.bsrnn_last_error().decode()
    assert lib.bsrnn_fir_stream_assign(st._h, i32s(0), 1, len(NAMES)) == EARG and "filter %d" % len(NAMES) in lib.bsrnn_last_error().decode()
    with pytest.raises(_native.NativeError):
        st.process(torch.zeros((2, 100)))                                    # a CPU tensor
    with pytest.raises(ValueError):
        st.process(torch.zeros((3, 100), device="cuda"))
    with pytest.raises(ValueError):
        st.assign([0], NAMES.index("j"))
    with pytest.raises(ValueError):
        FirStream(bank, 2, max_taps=0)
    if torch.cuda.device_count() > 1:
        other = torch.zeros((2, 2000), device="cuda:1")
        refused("lies on device", **{"in": ctypes.c_void_p(other.data_ptr())})
    torch.cuda.synchronize()
    assert list(n_out) == [-7, -7] and bool((b == SENTINEL).all())           # no refused call reported or wrote anything
    assert st.filter_of(0) == f and st.ready(0, 1000) == 1024                # ... or moved the stream
    parts.append(process(st, [x, x], at, [1900, 1900])[0])
    parts.append(flush(st, None, [owed_of(st, bank, r, 3000) for r in range(2)])[0])
    assert torch.equal(torch.cat(parts), oneshot[f])
