"""bsrnn_stream_process_hops on the GPU: one call in which every row of a bsrnn_stream advances by its own number of hops, and
StreamPool.feed on top of it.  A row is held to the StreamingOracle stepped over its own hops only, to the BITS of the same row in a
call where every row has all hops (rows do not see each other; the time axis is causal), and to a one-row twin stream at every count
and workgroup boundary.  The checks themselves live in tests/stream_hops_cases.py, which the other time-axis forms run in a child
process.  Bounds: TOL and STATE_TOL of tests/test_gpu_stream_block.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import stream_hops_cases as cases
from stream_hops_cases import HOP, NFFT, STATE_TOL, TOL, make_model, maxabs, t2n

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 1. the oracle, smallest mixed case
def test_smallest_mixed_case_against_the_oracle(sd_default):
    worst, worst_state = cases.smallest_mixed_case(sd_default)
    print("C = 4, L = 3, hops [3,1,2,0] then [0,2,1,3]: output %.3e (< %.0e), state %.3e (< %.0e)" % (worst, TOL, worst_state, STATE_TOL))


def test_41_bands_four_sequences_straddle_the_rows():
    """K = 42: sequences 40 .. 43 of the time-axis launch share a workgroup and belong to rows 0 and 1, which stop at different frames."""
    from speechseparation_amd import spec, weights
    v = spec.variant_bandsplits("41")
    sd = weights.synth_state_dict(v, seed=3)
    worst, worst_state = cases.oracle_case(sd, v, 2, 3, [[1, 3]], seed=91, label="41 bands")
    print("41 bands, C = 2, hops [1,3]: output %.3e, state %.3e" % (worst, worst_state))


# ------------------------------------------------------------------------------------------------ 2. rows do not see each other
@pytest.mark.parametrize("L,hops", [(3, [3, 1, 2, 0]), (19, [19, 5, 18, 0])])
def test_rows_do_not_see_each_other(sd_default, L, hops):
    from speechseparation_amd import weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    C = 4
    m = make_model(sd_default)
    a, b = StreamingSeparator(m, channels=C), StreamingSeparator(m, channels=C)
    wave = weights.synth_waveform(C, (2 + L) * HOP, seed=92)
    warm, x = cuda(wave[:, :2 * HOP]), cuda(wave[:, 2 * HOP:])
    assert torch.equal(a.process(warm), b.process(warm))                      # the same stream state, and not zero
    held = a.get_row(3)
    got_a = a.process_hops(cases.fed_with_nan(x, hops), hops)
    got_b = b.process_hops(x, [L] * C)                                        # every row all hops: the plain process, by delegation
    cases.check_zero_tail(got_a, hops, "A")
    assert torch.equal(got_a[0], got_b[0]), "row 0 (all hops in both calls) saw its neighbours' counts"
    assert torch.equal(a.get_row(0), b.get_row(0)), "carry of row 0"
    for r in (1, 2):
        n = hops[r]
        assert 0 < n < L
        assert torch.equal(got_a[r, :n * HOP], got_b[r, :n * HOP]), ("the hops a row has are not those of the full call", r, n)
        assert not torch.equal(a.get_row(r), b.get_row(r)), ("a row that stopped early has the carry of one that went on", r)
    assert torch.equal(a.get_row(3), held), "carry of the row without a hop"


# ------------------------------------------------------------------------------------------------ 3. held is held, and the delegation
def test_held_is_held_and_all_or_none_is_the_rows_call(sd_default):
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    C, L = 4, 3
    m = make_model(sd_default)
    st, twin = StreamingSeparator(m, channels=C), StreamingSeparator(m, channels=C)
    wave = weights.synth_waveform(C, (3 * L + 1) * HOP, seed=93)
    xs = [cuda(wave[:, i * L * HOP:(i + 1) * L * HOP]) for i in range(3)]
    one = cuda(wave[:, 3 * L * HOP:])
    mix_rows = torch.tensor([1.0, 0.3, -0.5, 1.0]).cuda()
    # every count 0 or L is the rows call with the matching flags, per-row mix included; one hop too (the step's kernels)
    for x, flags, mix in ((xs[0], [1, 1, 1, 1], 1.0), (xs[1], [1, 0, 0, 1], mix_rows), (one, [0, 1, 1, 0], 0.25), (xs[2], [0, 1, 1, 1], 1.0)):
        n = x.shape[1] // HOP
        got = st.process_hops(x, [n * f for f in flags], mix)
        assert torch.equal(got, twin.process_rows(x, flags, mix)), ("all-or-none counts are not the rows call", flags)
    for r in range(C):
        assert torch.equal(st.get_row(r), twin.get_row(r)), r
    # a row without a hop in a mixed call: carry bit for bit, zeros out
    before = [st.get_row(r) for r in range(C)]
    got = st.process_hops(cases.fed_with_nan(xs[0], [2, 0, 3, 0]), [2, 0, 3, 0], mix_rows)
    for r in (1, 3):
        assert torch.equal(st.get_row(r), before[r]), ("carry of a row without a hop changed", r)
        assert not bool(got[r].any()), r
    for r in (0, 2):
        assert not torch.equal(st.get_row(r), before[r]), r
    # nobody has a hop: out zeroed, the carry set not flipped (the state handle reads the same set, bit for bit)
    before, state = [st.get_row(r) for r in range(C)], st.state()
    got = st.process_hops(torch.full_like(xs[1], float("nan")), [0] * C)
    assert not bool(got.any()) and tuple(got.shape) == (C, L * HOP)
    assert torch.equal(st.state(), state)
    for r in range(C):
        assert torch.equal(st.get_row(r), before[r]), r
    # refusals that need a stream: a count outside [0, n_hops] names its row; the overlap rules
    lib = _native.lib
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty_like(xs[0])
    keep = st.get_row(2)
    for bad, row in (([1, 2, 4, 0], b"row 2"), ([1, -1, 3, 0], b"row 1")):
        assert lib.bsrnn_stream_process_hops(st._h, ptr(xs[0]), ptr(out), L, (ctypes.c_int32 * C)(*bad), None, ctypes.c_float(1.0), None) == 1
        assert row in lib.bsrnn_last_error() and b"bsrnn_stream_process_hops" in lib.bsrnn_last_error(), lib.bsrnn_last_error()
    cnt = (ctypes.c_int32 * C)(1, 2, 3, 0)
    assert lib.bsrnn_stream_process_hops(st._h, ptr(xs[0]), ptr(xs[0]), L, cnt, None, ctypes.c_float(1.0), None) == 1
    assert b"re-run" in lib.bsrnn_last_error() and b"bsrnn_stream_process_hops" in lib.bsrnn_last_error()
    assert lib.bsrnn_stream_process_hops(st._h, ptr(xs[0]), ptr(out), L, cnt, ptr(out), ctypes.c_float(1.0), None) == 1
    assert b"mix_rows_dev" in lib.bsrnn_last_error()
    assert list(cnt) == [1, 2, 3, 0]                                          # the caller's array: read, never written
    assert torch.equal(st.get_row(2), keep)


# ------------------------------------------------------------------------------------------------ 4. every count, every workgroup boundary
@pytest.fixture(scope="module")
def default_model(sd_default):
    return make_model(sd_default)


@pytest.mark.parametrize("i", range(len(cases.EVERY_COUNT)))
def test_every_count_and_workgroup_boundary(default_model, i):
    counts = sorted(c for call in cases.EVERY_COUNT for c in call)
    assert sorted(set(counts)) == list(range(41))                              # between them the six calls take every count 0 .. 40
    cases.twin_case(default_model, 8, 40, cases.EVERY_COUNT[i], cases.EVERY_COUNT_NEXT[i], seed=100 + i, label="call %d" % i)


# ------------------------------------------------------------------------------------------------ 5. the other time-axis forms
def run_child(env, names):
    e = dict(os.environ, PYTHONPATH=REPO, **env)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "stream_hops_cases.py")] + names, env=e, cwd=REPO, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "all cases hold" in r.stdout, (env, r.returncode, r.stdout[-3000:])


def test_eight_sequences_per_workgroup_straddle_the_rows():
    """BSRNN_TIME_SEQ8=1 (read at first use: a child process): at K = 12 the eight sequences of a workgroup belong to two rows."""
    run_child({"BSRNN_TIME_SEQ8": "1"}, ["smallest", "every_count"])


def test_exact_fp32_time_axis_kernel():
    """BSRNN_LSTM=f32 (read at first use: a child process): the exact-fp32 time-axis kernel's ragged form."""
    run_child({"BSRNN_LSTM": "f32"}, ["smallest", "every_count"])


def test_four_sequence_kernel_without_the_fused_fc():
    """BSRNN_GEMM=f32 with the fp16x2 recurrent layers (read at first use: a child process): the time-axis launch does not form the
    block's fc, which is the four-sequence kernel's other instantiation - the one that stores h1 itself."""
    run_child({"BSRNN_GEMM": "f32"}, ["smallest", "every_count"])


def test_range_rerun_keeps_the_counts(sd_default):
    """A loud row under the exact range policy: the call runs again on the exact-fp32 kernels from the untouched carry set, with the same
    counts, and returns 0."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    C, L, hops = 4, 3, [3, 1, 2, 0]
    m = make_model(sd_default)
    st = StreamingSeparator(m, channels=C)
    wave = weights.synth_waveform(C, 2 * L * HOP, seed=94)
    xs = [cuda(wave[:, i * L * HOP:(i + 1) * L * HOP]) for i in range(2)]
    oracles = [onp.StreamingOracle(sd_default, C=1) for _ in range(C)]
    st.process_hops(xs[0], [2, 3, 1, 1])
    for r, h in enumerate([2, 3, 1, 1]):
        for l in range(h):
            oracles[r].step(t2n(xs[0][r:r + 1, l * HOP:(l + 1) * HOP]))
    loud = cases.fed_with_nan(xs[1], hops)
    loud[0] *= 3e7                                           # far beyond what the fp16x2 path holds: the call runs again, exactly
    before = st.get_row(3)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.empty_like(loud)
    rc = _native.lib.bsrnn_stream_process_hops(st._h, ptr(loud), ptr(out), L, (ctypes.c_int32 * C)(*hops), None, ctypes.c_float(1.0), None)
    assert rc == 0, _native.lib.bsrnn_last_error()
    torch.cuda.synchronize()
    cases.check_zero_tail(out, hops, "re-run")
    assert torch.equal(st.get_row(3), before)
    for r in (1, 2):
        for l in range(hops[r]):
            e = maxabs(t2n(out[r, l * HOP:(l + 1) * HOP]), oracles[r].step(t2n(xs[1][r:r + 1, l * HOP:(l + 1) * HOP]))[0])
            print("re-run: row %d hop %d vs oracle %.3e" % (r, l, e))
            assert e < TOL, (r, l, e)
        blob = st.get_row(r)
        es = maxabs(cases.blob_state(blob), oracles[r].state)
        print("re-run: row %d state vs oracle %.3e" % (r, es))
        assert es < STATE_TOL, (r, es)
        assert maxabs(t2n(blob)[:NFFT], oracles[r].buf[0]) == 0.0


def test_overlapped_plan_with_mixed_counts(default_model):
    """C = 8, 32 hops (the shape of test_gpu_stream_rows.py::test_block_path_holds_rows): the overlapped dual path, whose consumers wait
    on frame groups of all rows - padding frames count - and whose second time-axis launch writes state on the auxiliary stream.  The
    plan is the default one, so this needs no child process."""
    assert set((0, 1, 15, 16, 17, 32)) <= set(cases.OVERLAP_COUNTS)
    cases.twin_case(default_model, 8, 32, cases.OVERLAP_COUNTS, cases.OVERLAP_NEXT, seed=97, label="overlap", need_overlap=True)


# ------------------------------------------------------------------------------------------------ 6. no first-use work
def test_no_first_use_work_after_reserve(sd_default):
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    C, L = 4, 6
    m = make_model(sd_default)
    st = StreamingSeparator(m, channels=C)
    st.reserve(L)
    torch.cuda.synchronize()
    counters = lambda: tuple(_native.lib.bsrnn_debug_counter(i) for i in range(3))    # allocations, captures, instantiations
    ready = counters()
    wave = weights.synth_waveform(C, L * HOP, seed=95)
    mix_rows = torch.tensor([1.0, 0.5, 1.0, -0.25]).cuda()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for n, hops, mr in ((6, [6, 1, 0, 3], None), (6, [0, 5, 5, 2], mix_rows), (4, [1, 2, 3, 4], None), (2, [1, 0, 2, 1], mix_rows), (6, [5, 5, 5, 5], None)):
        x = cuda(wave[:, :n * HOP])
        out = torch.empty_like(x)
        rc = _native.lib.bsrnn_stream_process_hops(st._h, ptr(x), ptr(out), n, (ctypes.c_int32 * C)(*hops), ptr(mr) if mr is not None else None,
                                                   ctypes.c_float(1.0), None)
        assert rc == 0, _native.lib.bsrnn_last_error()
    torch.cuda.synchronize()
    assert counters() == ready, ("a hops call allocated, captured or instantiated after reserve", ready, counters())
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ 7. StreamPool.feed end to end
def test_stream_pool_feed_end_to_end(sd_default):
    from speechseparation_amd.bsrnn import StreamingSeparator, StreamPool
    from speechseparation_amd import weights
    m = make_model(sd_default)
    pool = StreamPool(m, 3, rows_per_session=2)
    # samples per tick and session: 0, 700, 1024, 2500 and 3 * 1024 all occur, and the sessions differ in every tick
    ticks = {"a": [700, 1024, 0, 2500, 3072, 100, 1024, 700],
             "b": [3072, 0, 700, 1024, 2500, 2500, 0, 1348],
             "c": [1024, 2500, 3072, 0, 700, 1024, 3072, 24]}
    audio = {n: weights.synth_waveform(2, sum(t), seed=110 + i) for i, (n, t) in enumerate(ticks.items())}
    sid = {n: pool.open() for n in ticks}
    pos = {n: 0 for n in ticks}
    got = {n: [] for n in ticks}
    calls = [0]
    for t in range(8):
        chunks = {}
        for n in ticks:
            chunks[sid[n]] = cuda(audio[n][:, pos[n]:pos[n] + ticks[n][t]])
            pos[n] += ticks[n][t]
        st = pool._stream()
        if t == 0:
            inner = st.process_hops
            def counted(*a, **k):
                calls[0] += 1
                return inner(*a, **k)
            st.process_hops = counted
        outs = pool.feed(chunks)
        assert sorted(outs) == sorted(sid.values())
        for n in ticks:
            o = outs[sid[n]]
            assert o.is_cuda and o.shape[0] == 2 and o.shape[1] % HOP == 0
            got[n].append(o)
            assert pool.pending(sid[n]) == (pos[n] % HOP)
    assert calls[0] == 8, calls                                                # one library call per feed
    worst = 0.0
    for n in ticks:
        y = torch.cat(got[n], 1)
        total = sum(ticks[n])
        assert y.shape[1] == (total // HOP) * HOP
        twin = StreamingSeparator(m, channels=2)
        ref = twin.process(cuda(audio[n]))
        e = maxabs(t2n(y), t2n(ref))
        worst = max(worst, e)
        assert e < STATE_TOL, ("session against its two-row twin", n, e)
    print("StreamPool.feed: 3 sessions x 8 ticks against two-row twins: %.3e (< %.0e)" % (worst, STATE_TOL))
    # a session closed and reopened starts fresh: no pending samples, silence behind it
    assert pool.pending(sid["b"]) > 0
    pool.close(sid["b"])
    again = pool.open()
    assert pool.pending(again) == 0
    x = cuda(audio["b"][:, :2 * HOP])
    fresh = StreamingSeparator(m, channels=2)
    e = maxabs(t2n(pool.feed({again: x})[again]), t2n(fresh.process(x)))
    assert e < STATE_TOL, e
