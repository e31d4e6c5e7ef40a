"""The native session pool on the GPU (bsrnn_pool_*, NativeStreamPool): one library call per tick of many live sessions.  The pool makes
the hops calls StreamPool makes, on the same samples, so it is held to StreamPool's BITS tick by tick, to an 8-row
StreamingSeparator.process_hops twin called with the rounds the plan prescribes, and - through them - to two-row twins within
STATE_TOL (tests/stream_hops_cases.py).  4 slots x 2 rows (C = 8), three sessions open, the default 12-band synthetic model."""
import ctypes

import numpy as np
import pytest
import torch

from stream_hops_cases import HOP, STATE_TOL, make_model, maxabs, t2n

pytestmark = pytest.mark.gpu

EARG = 1
# samples per tick and session: the script of test_gpu_stream_hops.py::test_stream_pool_feed_end_to_end
TICKS = {"a": [700, 1024, 0, 2500, 3072, 100, 1024, 700],
         "b": [3072, 0, 700, 1024, 2500, 2500, 0, 1348],
         "c": [1024, 2500, 3072, 0, 700, 1024, 3072, 24]}


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def counters():
    from speechseparation_amd import _native
    return tuple(_native.lib.bsrnn_debug_counter(i) for i in range(3))         # allocations, captures, instantiations


def native_pool(m, max_hops=3, sessions=3):
    from speechseparation_amd.bsrnn import NativeStreamPool
    pool = NativeStreamPool(m, 4, rows_per_session=2, max_hops=max_hops)
    return pool, [pool.open() for _ in range(sessions)]


def python_pool(m, sessions=3):
    from speechseparation_amd.bsrnn import StreamPool
    pool = StreamPool(m, 4, rows_per_session=2)
    return pool, [pool.open() for _ in range(sessions)]


def raw_feed(pool, sids, ins, outs, n_in=None, mix=None, host=False):
    """bsrnn_pool_feed itself: ins / outs are tensors [2, n] (any strides) or None; -> (rc, n_out list)."""
    from speechseparation_amd import _native
    n = len(sids)
    stride = lambda t: 0 if t is None else (t.stride(0) if t.shape[0] > 1 else t.shape[1])
    slots = (ctypes.c_int32 * n)(*[pool._slot[s] if s in pool._slot else s for s in sids])
    in_p = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ins])
    in_s = (ctypes.c_int64 * n)(*[stride(t) for t in ins])
    cnt = (ctypes.c_int64 * n)(*(n_in if n_in is not None else [0 if t is None else t.shape[1] for t in ins]))
    out_p = (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in outs])
    out_s = (ctypes.c_int64 * n)(*[stride(t) for t in outs])
    got = (ctypes.c_int64 * n)(*([-1] * n))
    mix_p = None if mix is None else (ctypes.c_float * n)(*mix)
    h = pool._pool()
    if host:
        rc = _native.lib.bsrnn_pool_feed_host(h, n, slots, in_p, in_s, cnt, out_p, out_s, got, mix_p, ctypes.c_float(1.0))
    else:
        rc = _native.lib.bsrnn_pool_feed(h, n, slots, in_p, in_s, cnt, out_p, out_s, got, mix_p, ctypes.c_float(1.0),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, list(got)


@pytest.fixture(scope="module")
def model(sd_default):
    return make_model(sd_default)


@pytest.fixture(scope="module")
def audio():
    from speechseparation_amd import weights
    return {n: weights.synth_waveform(2, sum(t), seed=110 + i) for i, (n, t) in enumerate(TICKS.items())}


def script_chunks(audio, t):
    pos = {n: sum(TICKS[n][:t]) for n in TICKS}
    return {n: audio[n][:, pos[n]:pos[n] + TICKS[n][t]] for n in TICKS}


@pytest.fixture(scope="module")
def script_run(model, audio):
    """The 8-tick script through StreamPool, then through a NativeStreamPool (max_hops = 3) with the first-use counters read after its
    creation and after its last feed.  Computed once; tests 1, 4 and 8 read it."""
    ref_pool, ref_sid = python_pool(model)
    ref = []
    for t in range(8):
        ch = script_chunks(audio, t)
        outs = ref_pool.feed({s: cuda(ch[n]) for s, n in zip(ref_sid, TICKS)})
        ref.append(({n: outs[s] for s, n in zip(ref_sid, TICKS)}, {n: ref_pool.pending(s) for s, n in zip(ref_sid, TICKS)}))
    pool, sid = native_pool(model, max_hops=3)
    pool._pool()
    torch.cuda.synchronize()
    ready = counters()
    got = []
    for t in range(8):
        ch = script_chunks(audio, t)
        outs = pool.feed({s: cuda(ch[n]) for s, n in zip(sid, TICKS)})
        got.append(({n: outs[s] for s, n in zip(sid, TICKS)}, {n: pool.pending(s) for s, n in zip(sid, TICKS)}))
    torch.cuda.synchronize()
    return {"ref": ref, "got": got, "ready": ready, "after": counters()}


# ------------------------------------------------------------------------------------------------ 1. tick by tick against StreamPool
def test_tick_by_tick_equal_to_stream_pool(model, audio, script_run):
    from speechseparation_amd.bsrnn import StreamingSeparator
    for t in range(8):
        (ref, ref_pend), (got, pend) = script_run["ref"][t], script_run["got"][t]
        for n in TICKS:
            assert got[n].is_cuda and got[n].shape == ref[n].shape and got[n].shape[1] % HOP == 0, (t, n, got[n].shape, ref[n].shape)
            assert torch.equal(got[n], ref[n]), ("tick against StreamPool", t, n, maxabs(t2n(got[n]), t2n(ref[n])))
            assert pend[n] == ref_pend[n] == sum(TICKS[n][:t + 1]) % HOP, (t, n, pend[n], ref_pend[n])
    worst = 0.0
    for n in TICKS:
        y = torch.cat([script_run["got"][t][0][n] for t in range(8)], 1)
        assert y.shape[1] == (sum(TICKS[n]) // HOP) * HOP
        e = maxabs(t2n(y), t2n(StreamingSeparator(model, channels=2).process(cuda(audio[n]))))
        worst = max(worst, e)
        print("session %s against its two-row twin: %.3e" % (n, e))
        assert e < STATE_TOL, ("session against its two-row twin", n, e)
    print("NativeStreamPool.feed: 3 sessions x 8 ticks: equal to StreamPool, two-row twins within %.3e (< %.0e)" % (worst, STATE_TOL))


# ------------------------------------------------------------------------------------------------ 2. rounds
def test_rounds_at_max_hops_2(model, audio):
    from speechseparation_amd.bsrnn import StreamingSeparator
    pool, sid = native_pool(model, max_hops=2, sessions=2)
    xa, xb = cuda(audio["a"][:, :5 * HOP + 300]), cuda(audio["b"][:, :HOP])
    outs = pool.feed({sid[0]: xa, sid[1]: xb})
    assert outs[sid[0]].shape == (2, 5 * HOP) and outs[sid[1]].shape == (2, HOP)
    assert pool.pending(sid[0]) == 300 and pool.pending(sid[1]) == 0
    # the rounds the plan prescribes, as hops calls of an 8-row stream: counts 2 / 2 / 1 for rows 0-1 and 1 / 0 / 0 for rows 2-3
    twin = StreamingSeparator(model, channels=8)
    ya, yb, done = [], [], 0
    for ha, hb in ((2, 1), (2, 0), (1, 0)):
        L = max(ha, hb)
        wave = torch.zeros((8, L * HOP), device="cuda")
        wave[0:2, :ha * HOP] = xa[:, done * HOP:(done + ha) * HOP]
        wave[2:4, :hb * HOP] = xb[:, :hb * HOP]
        out = twin.process_hops(wave, [ha, ha, hb, hb, 0, 0, 0, 0])
        ya.append(out[0:2, :ha * HOP])
        yb.append(out[2:4, :hb * HOP])
        done += ha
    assert torch.equal(outs[sid[0]], torch.cat(ya, 1)), maxabs(t2n(outs[sid[0]]), t2n(torch.cat(ya, 1)))
    assert torch.equal(outs[sid[1]], torch.cat(yb, 1))
    for o, x, n in ((outs[sid[0]], xa, 5), (outs[sid[1]], xb, 1)):
        e = maxabs(t2n(o), t2n(StreamingSeparator(model, channels=2).process(x[:, :n * HOP].contiguous())))
        print("rounds: %d hops against a two-row twin: %.3e" % (n, e))
        assert e < STATE_TOL, (n, e)
    # what waits is the 300 samples behind the fifth hop: one more feed completes the sixth
    more = cuda(audio["a"][:, 5 * HOP + 300:6 * HOP])
    o6 = pool.feed({sid[0]: more})[sid[0]]
    assert o6.shape == (2, HOP) and pool.pending(sid[0]) == 0
    wave = torch.zeros((8, HOP), device="cuda")
    wave[0:2] = cuda(audio["a"][:, 5 * HOP:6 * HOP])
    assert torch.equal(o6, twin.process_hops(wave, [1, 1, 0, 0, 0, 0, 0, 0])[0:2])


# ------------------------------------------------------------------------------------------------ 3. arbitrary pointers
def test_arbitrary_pointers_and_strides(model, audio):
    nan = float("nan")
    plain, psid = native_pool(model)
    pool, sid = native_pool(model)
    for t in (0, 1, 3):                                   # pending 0 and not 0; 0, 1, 2 and 3 hops; a session that brings nothing
        ch = script_chunks(audio, t)
        want = plain.feed({s: cuda(ch[n]) for s, n in zip(psid, TICKS)})
        ins, outs, n_out = [], [], []
        for s, n in zip(sid, TICKS):
            k = ch[n].shape[1]
            if k == 0:
                ins.append(None)                          # nothing to read: a null pointer is fine
            else:
                base = torch.full((2 * (k + 37) + 1,), nan, device="cuda")
                view = base[1:].view(2, k + 37)[:, :k]    # a storage offset of one float, a row stride above n, NaN around the windows
                view.copy_(cuda(ch[n]))
                assert view.data_ptr() % 16 == 4 and view.stride(0) == k + 37
                ins.append(view)
            m = (pool.pending(s) + k) // HOP * HOP
            n_out.append(m)
            buf = torch.full((2 * (m + 5) + 3,), nan, device="cuda")
            outs.append(buf[3:].view(2, m + 5))           # (the whole padded rows: what lies behind n_out must stay NaN)
        rc, got = raw_feed(pool, sid, ins, outs)
        assert rc == 0 and got == n_out, (rc, got, n_out)
        torch.cuda.synchronize()
        for s, ps, o, m in zip(sid, psid, outs, n_out):
            assert torch.equal(o[:, :m], want[ps]), ("strided against contiguous", t, s)
            assert bool(torch.isnan(o[:, m:]).all()), ("written behind n_out", t, s)
            assert pool.pending(s) == plain.pending(ps)


# ------------------------------------------------------------------------------------------------ 4. the host form
def test_host_form_equals_the_device_form(model, audio, script_run):
    pool, sid = native_pool(model)
    for t in range(8):
        ch = script_chunks(audio, t)
        outs = pool.feed({s: torch.from_numpy(np.ascontiguousarray(ch[n])) for s, n in zip(sid, TICKS)})
        got, pend = script_run["got"][t]
        for s, n in zip(sid, TICKS):
            assert not outs[s].is_cuda and outs[s].shape == got[n].shape
            assert torch.equal(outs[s], got[n].cpu()), ("host form against device form", t, n)
            assert pool.pending(s) == pend[n]


# ------------------------------------------------------------------------------------------------ 5. mix
def test_mix_equals_stream_pool(model, audio):
    pool, sid = native_pool(model)
    ref, rsid = python_pool(model)
    plain, psid = native_pool(model)
    # the wet / dry control reaches a session's carry (its previous synthesis frame), so a session is held to the plain pool's bits only
    # while it has never been mixed itself: session 2 in ticks 0 and 1, beside sessions at 0.5 that have hops
    mixed = set()
    beside = 0
    for t, mix in ((0, {1: 0.5, 2: 1.0}), (1, {0: 0.5}), (3, {0: 0.5, 2: -0.25}), (4, 0.5), (5, None)):
        ch = script_chunks(audio, t)
        as_mix = lambda ids: {ids[k]: v for k, v in mix.items()} if isinstance(mix, dict) else mix
        got = pool.feed({s: cuda(ch[n]) for s, n in zip(sid, TICKS)}, as_mix(sid))
        want = ref.feed({s: cuda(ch[n]) for s, n in zip(rsid, TICKS)}, as_mix(rsid))
        dry = plain.feed({s: cuda(ch[n]) for s, n in zip(psid, TICKS)})
        for k in range(3):
            assert torch.equal(got[sid[k]], want[rsid[k]]), ("mix against StreamPool", t, k)
            value = 1.0 if mix is None else (mix.get(k, 1.0) if isinstance(mix, dict) else mix)
            if value != 1.0:
                mixed.add(k)
            if k not in mixed:                            # a session at 1.0 beside one at 0.5 gets the plain call's bits
                assert torch.equal(got[sid[k]], dry[psid[k]]), ("a session at 1.0", t, k)
                beside += bool(got[sid[k]].shape[1]) and isinstance(mix, dict)
            elif value != 1.0 and got[sid[k]].shape[1]:
                assert not torch.equal(got[sid[k]], dry[psid[k]]), ("the mix did nothing", t, k)
    assert beside >= 2


# ------------------------------------------------------------------------------------------------ 6. held, closed and reopened sessions
def test_held_closed_and_reopened_sessions(model, audio):
    pool, sid = native_pool(model)
    ref, rsid = python_pool(model)
    named = {0: (0, 1, 2), 1: (0, 2), 2: (2,), 3: (0, 1, 2), 4: (1,), 5: (0, 1, 2)}      # session 1 sits out ticks 1-2, session 0 tick 2 and 4
    pos = [0, 0, 0]
    for t in range(6):
        feed, rfeed = {}, {}
        for k in named[t]:
            n = "abc"[k]
            x = cuda(audio[n][:, pos[k]:pos[k] + TICKS[n][t]])
            pos[k] += TICKS[n][t]
            feed[sid[k]], rfeed[rsid[k]] = x, x
        got, want = pool.feed(feed), ref.feed(rfeed)
        for k in named[t]:
            assert torch.equal(got[sid[k]], want[rsid[k]]), ("a session that was held", t, k)
        for k in range(3):
            assert pool.pending(sid[k]) == ref.pending(rsid[k]) == pos[k] % HOP
    # closed and reopened: the first hops of a fresh stream, nothing waiting
    assert pool.pending(sid[1]) > 0
    slot = pool._slot[sid[1]]
    pool.close(sid[1])
    again = pool.open()
    assert pool._slot[again] == slot and pool.pending(again) == 0
    fresh, fsid = native_pool(model, sessions=2)
    x = cuda(audio["b"][:, :2 * HOP + 10])
    assert torch.equal(pool.feed({again: x})[again], fresh.feed({fsid[1]: x})[fsid[1]])
    assert pool.pending(again) == 10


# ------------------------------------------------------------------------------------------------ 7. moving a session in the middle of a hop
def test_moving_mid_hop(model, audio):
    a, asid = native_pool(model, sessions=1)
    b, _ = native_pool(model, sessions=2)
    whole, wsid = native_pool(model, sessions=1)
    x = cuda(audio["c"])
    cuts = [0, 700, 2048, 3548, 5548]
    want = [whole.feed({wsid[0]: x[:, cuts[i]:cuts[i + 1]]})[wsid[0]] for i in range(4)]
    assert [w.shape[1] for w in want] == [0, 2 * HOP, HOP, 2 * HOP]
    assert a.feed({asid[0]: x[:, :700]})[asid[0]].shape == (2, 0) and a.pending(asid[0]) == 700
    blobs, pending = a.export(asid[0])
    assert len(blobs) == 2 and pending.shape == (2, 700) and torch.equal(pending, x[:, :700].cpu())
    moved = b.adopt(blobs, pending)
    assert b._slot[moved] == 2 and b.pending(moved) == 700
    assert torch.equal(b.feed({moved: x[:, 700:2048]})[moved], want[1]), "moved after 700 samples, fed 1348 more"
    # and back, with a carry that is no longer silence and 476 samples waiting
    assert torch.equal(b.feed({moved: x[:, 2048:3548]})[moved], want[2]) and b.pending(moved) == 476
    back = a.adopt(*b.export(moved))
    assert a.pending(back) == 476
    assert torch.equal(a.feed({back: x[:, 3548:5548]})[back], want[3])
    assert a.pending(back) == whole.pending(wsid[0]) == 5548 % HOP


# ------------------------------------------------------------------------------------------------ 8. no first-use work
def test_no_first_use_work_after_create(script_run):
    assert script_run["after"] == script_run["ready"], ("a feed allocated, captured or instantiated", script_run["ready"], script_run["after"])


# ------------------------------------------------------------------------------------------------ 9. refusals that need a pool
def test_refusals_leave_the_pool_untouched(model, audio):
    from speechseparation_amd import _native
    pool, sid = native_pool(model)
    twin, tsid = native_pool(model)
    ch = script_chunks(audio, 1)                              # 1024 / 0 / 2500 samples
    first = {n: cuda(ch[n]) for n in TICKS}
    for p, ids in ((pool, sid), (twin, tsid)):
        p.feed({s: first[n] for s, n in zip(ids, TICKS)})     # something waits: 0 / 0 / 452 samples
    x = cuda(audio["a"][:, :2 * HOP + 100])
    out = torch.empty((2, 2 * HOP), device="cuda")

    def refused(rc, *words):
        assert rc == EARG, (rc, _native.lib.bsrnn_last_error())
        for w in ("bsrnn_pool_feed",) + words:
            assert w.encode() in _native.lib.bsrnn_last_error(), (w, _native.lib.bsrnn_last_error())
    # a slot named twice: the second mention, session 1, is named
    refused(raw_feed(pool, [sid[0], sid[0]], [x, x], [out, torch.empty_like(out)])[0], "session 1", "slot 0")
    # a closed slot (slot 3 was never opened)
    refused(raw_feed(pool, [sid[1], 3], [x, x], [out, torch.empty_like(out)])[0], "session 1", "slot 3", "not open")
    # out_stride below the session's n_out
    tight = torch.empty((2, HOP), device="cuda")
    refused(raw_feed(pool, [sid[1], sid[0]], [None, x], [None, tight])[0], "session 1", "out_stride")
    # an output of the call over an input of the call: session 0 would write where session 2 reads
    both = torch.zeros((2, 4 * HOP), device="cuda")
    refused(raw_feed(pool, [sid[0], sid[2]], [x, both[:, HOP:3 * HOP]], [both[:, :2 * HOP], out])[0], "session 0", "session 1", "slot 2", "overlaps")
    # in place
    y = x.clone()
    refused(raw_feed(pool, [sid[0]], [y], [y])[0], "session 0", "overlaps")
    # a stride below its count, a negative count
    refused(raw_feed(pool, [sid[0]], [x[:, :HOP]], [out], n_in=[3 * HOP])[0], "session 0", "in_stride")
    refused(raw_feed(pool, [sid[0]], [x], [out], n_in=[-1])[0], "session 0", "n_in")
    torch.cuda.synchronize()
    assert torch.equal(y, x), "a refused call wrote"
    for s, ts in zip(sid, tsid):
        assert pool.pending(s) == twin.pending(ts)
    ch = script_chunks(audio, 2)
    got = pool.feed({s: cuda(ch[n]) for s, n in zip(sid, TICKS)})
    want = twin.feed({s: cuda(ch[n]) for s, n in zip(tsid, TICKS)})
    for s, ts in zip(sid, tsid):
        assert torch.equal(got[s], want[ts]) and pool.pending(s) == twin.pending(ts)


# ------------------------------------------------------------------------------------------------ 10. the range re-run
def test_range_rerun_consumes_the_fifo_once(model, audio):
    """Exact range policy (the default): a loud session leaves the fp16 range, the hops call runs again on the exact kernels.  The gather
    launch wrote the FIFO before the first run; the re-run reads the pool's rectangle, so nothing is consumed twice."""
    pool, sid = native_pool(model)
    ref, rsid = python_pool(model)
    x = {n: cuda(audio[n][:, :5000]) for n in TICKS}
    cuts = {"a": (700, 2800), "b": (1100, 3400), "c": (0, 1500)}
    for p, ids in ((pool, sid), (ref, rsid)):
        p.feed({s: x[n][:, :cuts[n][0]] for s, n in zip(ids, TICKS)})          # 700 / 76 / 0 samples wait
    loud = {n: x[n][:, cuts[n][0]:cuts[n][1]].clone() for n in TICKS}
    loud["a"] *= 3e7                                          # far beyond what the fp16x2 path holds
    got = pool.feed({s: loud[n] for s, n in zip(sid, TICKS)})
    want = ref.feed({s: loud[n] for s, n in zip(rsid, TICKS)})
    for s, rs, n in zip(sid, rsid, TICKS):
        assert got[s].shape[1] == (cuts[n][1] // HOP) * HOP - (cuts[n][0] // HOP) * HOP
        assert bool(torch.isfinite(got[s]).all())
        assert torch.equal(got[s], want[rs]), ("re-run against StreamPool", n)
        assert pool.pending(s) == ref.pending(rs) == cuts[n][1] % HOP
    # what waited went in once: the next tick still agrees
    got = pool.feed({s: x[n][:, cuts[n][1]:] for s, n in zip(sid, TICKS)})
    want = ref.feed({s: x[n][:, cuts[n][1]:] for s, n in zip(rsid, TICKS)})
    for s, rs in zip(sid, rsid):
        assert got[s].shape[1] > 0 and torch.equal(got[s], want[rs])
