"""GPU: StreamPool sessions at their own sample rates (StreamPool(rates=...), open(sample_rate=...), feed, drain).  The pool with its two
resampler banks is held to the COMPOSITION it replaces - a pool without rates, surrounded by one single-pair Resampler per session and
direction - and since both hand the same converted chunks to the same feed code, both make the same bsrnn_stream_process_hops calls:
every expectation is an equality (torch.equal), there is no tolerance.  What a bank row computes is tests/test_gpu_resample_bank.py's."""
import numpy as np
import pytest
import torch

from stream_hops_cases import HOP, make_model

pytestmark = pytest.mark.gpu
MODEL_RATE = 44100
# session-rate samples per tick: 0, 700, 1 115, 2 700 and 3 300 all occur, in another order per session
TICKS = {"a": (48000, 0, [700, 2700, 0, 3300, 1115, 700]),
         "b": (16000, 0, [1115, 0, 3300, 700, 2700, 1115]),
         "c": (None, 0, [2700, 1115, 700, 0, 3300, 2700]),
         "d": (48000, 2, [0, 0, 3300, 1115, 0, 2700])}          # opened at tick 2


@pytest.fixture(scope="module")
def model(sd_default):
    return make_model(sd_default)


def audio(name, n):
    return torch.from_numpy(0.1 * np.random.default_rng(sum(map(ord, name))).standard_normal((2, n)).astype(np.float32)).cuda()


class Composition:
    """A session of a pool WITHOUT rates, with the test's own single-pair resamplers around it: the steps StreamPool documents."""

    def __init__(self, model, pool, rate):
        from speechseparation_amd.bsrnn import Resampler
        self.pool, self.rate = pool, rate
        self.sid = pool.open()
        self.skip = HOP                                                  # the stream's one-hop delay, dropped from the session's audio
        if rate is not None:
            self.rin, self.rout = Resampler(model, 2, rate, MODEL_RATE), Resampler(model, 2, MODEL_RATE, rate)

    def inbound(self, chunk):
        return chunk if self.rate is None else self.rin.process(chunk)

    def outbound(self, out):
        if self.rate is None:
            return out
        k = min(self.skip, out.shape[1])
        self.skip -= k
        return self.rout.process(out[:, k:].contiguous())

    def drain(self):
        if self.rate is None:
            x = torch.empty((2, 0), device="cuda")
        else:
            x = self.rin.flush()                                         # 1. the inbound rows are flushed
        pad = -(self.pool.pending(self.sid) + x.shape[1]) % HOP          # 2. zeros to a whole hop, 3. one more hop for the delay
        x = torch.cat((x, torch.zeros((2, pad + HOP), device="cuda")), 1)
        out = self.pool.feed({self.sid: x})[self.sid]                    # 4. those hops, everyone else held
        assert self.pool.pending(self.sid) == 0
        if self.rate is None:
            return out
        return torch.cat((self.outbound(out), self.rout.flush()), 1)     # 5. outbound process, then flush


def test_the_pool_equals_the_composition_and_the_lengths_follow_the_rule(model):
    from speechseparation_amd.bsrnn import StreamPool, resample_len
    A = StreamPool(model, 4, 2, rates=(16000, 48000))
    B = StreamPool(model, 4, 2)
    clips = {n: audio(n, sum(t[2])) for n, t in TICKS.items()}
    sid, comp, pos, received = {}, {}, {n: 0 for n in TICKS}, {n: 0 for n in TICKS}
    hops_calls = [0]
    for tick in range(6):
        for n, (rate, first, _) in TICKS.items():
            if first == tick:
                sid[n] = A.open(sample_rate=rate)
                comp[n] = Composition(model, B, rate)
                assert A._slot[sid[n]] == B._slot[comp[n].sid]
        chunks = {}
        for n in sid:
            k = TICKS[n][2][tick]
            chunks[n] = clips[n][:, pos[n]:pos[n] + k]
            pos[n] += k
        got = A.feed({sid[n]: c for n, c in chunks.items()})
        if tick == 0:                                                    # one process_hops per feed, with the banks around it
            inner = A._st.process_hops

            def counted(*a, **k):
                hops_calls[0] += 1
                return inner(*a, **k)
            A._st.process_hops = counted
        ref = B.feed({comp[n].sid: comp[n].inbound(c) for n, c in chunks.items()})
        for n in sid:
            want = comp[n].outbound(ref[comp[n].sid])
            y = got[sid[n]]
            assert y.is_cuda and tuple(y.shape) == tuple(want.shape) and torch.equal(y, want), ("session against the composition", tick, n)
            assert A.pending(sid[n]) == B.pending(comp[n].sid) < HOP          # samples at the model's rate
            received[n] += y.shape[1]
    assert hops_calls[0] == 5, hops_calls
    assert A._bank_in is not None and B._bank_in is None and B._bank_out is None
    assert received["c"] == (sum(TICKS["c"][2]) // HOP) * HOP
    for n in ("a", "c", "b", "d"):
        tail = A.drain(sid[n])
        want = comp[n].drain()
        assert tuple(tail.shape) == tuple(want.shape) and torch.equal(tail, want), ("drain against the composition", n)
        rate, fed = TICKS[n][0], sum(TICKS[n][2])
        assert A.pending(sid[n]) == 0
        if rate is None:
            assert received[n] + tail.shape[1] == -(-fed // HOP) * HOP + HOP          # the padded hops and the extra one, as the stream gives them
        else:
            m = -(-resample_len(fed, rate, MODEL_RATE) // HOP) * HOP
            assert received[n] + tail.shape[1] == resample_len(m, MODEL_RATE, rate), ("the length rule of drain()", n)
    # a drained session starts a new piece of audio, as a fresh one does
    for n in ("a", "b"):
        B._stream().reset_rows(list(B._rows_of(comp[n].sid)))
        comp[n].skip = HOP
        x = clips[n][:, :2700]
        y = A.feed({sid[n]: x})[sid[n]]
        want = comp[n].outbound(B.feed({comp[n].sid: comp[n].inbound(x)})[comp[n].sid])
        assert y.shape[1] > 0 and torch.equal(y, want), ("after drain", n)


def test_step_refuses_a_session_with_a_rate(model):
    from speechseparation_amd.bsrnn import StreamPool
    pool = StreamPool(model, 2, 2, rates=(48000,))
    a, b = pool.open(sample_rate=48000), pool.open()
    hop = torch.zeros((2, HOP), device="cuda")
    with pytest.raises(ValueError, match=r"feed\(\)"):
        pool.step({a: hop, b: hop})
    out = pool.step({b: hop})
    assert sorted(out) == [b] and tuple(out[b].shape) == (2, HOP)
    with pytest.raises(ValueError):
        pool.export(a)
    assert len(pool.export(b)) == 2


def test_close_lets_the_rows_start_afresh(model):
    """A session at 48 kHz leaves mid-stream; the slot's next session, at 16 kHz, equals the same session in a fresh pool."""
    from speechseparation_amd.bsrnn import StreamPool
    used, fresh = StreamPool(model, 2, 2, rates=(16000, 48000)), StreamPool(model, 2, 2, rates=(16000, 48000))
    a = used.open(sample_rate=48000)
    assert used.feed({a: audio("x", 3300)})[a].shape[1] > 0
    assert used.pending(a) > 0
    used.close(a)
    s, t = used.open(sample_rate=16000), fresh.open(sample_rate=16000)
    assert used._slot[s] == fresh._slot[t] == 0 and used.pending(s) == 0
    x = audio("y", 3000)
    for lo, hi in ((0, 1115), (1115, 1115), (1115, 3000)):
        y, want = used.feed({s: x[:, lo:hi]})[s], fresh.feed({t: x[:, lo:hi]})[t]
        assert torch.equal(y, want)
    y, want = used.drain(s), fresh.drain(t)
    assert y.shape[1] > 0 and torch.equal(y, want)


def test_banks_are_optional(model, sd_default):
    """A pool without rates makes no bank: its first feed allocates what the stream's own flow allocates for the same calls."""
    from speechseparation_amd import _native
    from speechseparation_amd.bsrnn import StreamingSeparator, StreamPool
    count = lambda: _native.lib.bsrnn_debug_counter(0)
    x = audio("z", 2 * HOP)
    model.separate(x)                        # (this process has had a context before: what is counted below is per context)
    # the flow as it was: a stream of 4 rows and one process_hops
    m = make_model(sd_default)
    torch.cuda.synchronize()
    before = count()
    st = StreamingSeparator(m, channels=4)
    wave = torch.zeros((4, 2 * HOP), device="cuda")
    wave[0:2] = x
    st.process_hops(wave, [2, 2, 0, 0])
    torch.cuda.synchronize()
    plain = count() - before
    # the pool, without rates
    m = make_model(sd_default)
    torch.cuda.synchronize()
    before = count()
    pool = StreamPool(m, 2, 2)
    a = pool.open()
    out = pool.feed({a: x})[a]
    torch.cuda.synchronize()
    assert count() - before == plain, ("a pool without rates allocated something the stream's own flow does not", count() - before, plain)
    assert pool._bank_in is None and pool._bank_out is None and tuple(out.shape) == (2, 2 * HOP)
    # ... and with rates the banks come with the stream: two objects, and the tables of the pairs
    m = make_model(sd_default)
    torch.cuda.synchronize()
    before = count()
    pool = StreamPool(m, 2, 2, rates=(48000,))
    a = pool.open()
    pool.feed({a: x})
    torch.cuda.synchronize()
    assert count() - before == plain + 4 and pool._bank_in is not None          # two banks, two tables (48 -> 44.1 k, 44.1 -> 48 k)
