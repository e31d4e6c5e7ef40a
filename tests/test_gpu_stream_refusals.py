"""GPU: what the streaming layer refuses once a stream exists, and the library calls a pool's tick makes.
First the exact text of the refusals of StreamingSeparator.process_rows / process_hops / set_row / get_row / reset_rows (2 channels) and
of a ResamplerBank (2 rows on 48 k -> 44.1 k).  Then one fixed script - open, feed, step, drain, export / adopt, close - on a StreamPool
and on a NativeRatePool of 3 slots x 1 row with rates = (48000,), behind a proxy that records the NAME of every library call: the list
must be the one written out below.  Numbers are not compared here: tests/test_gpu_stream_pool_rates.py, test_gpu_pool_native.py and
test_gpu_pool_native_rates.py hold the pools to StreamingSeparator bit for bit.  tests/test_stream_refusals_host.py holds the refusals
that need no device."""
import sys

import pytest
import torch

from stream_hops_cases import HOP, make_model

pytestmark = pytest.mark.gpu

# The library calls of script() below, *_destroy left out (those are made when objects are collected, which is not the script's doing).
# Recorded on the commit before the streaming classes left bsrnn.py (d6ca072).
STREAM_POOL_CALLS = [
    "bsrnn_resample_len", "bsrnn_stream_create", "bsrnn_resample_len", "bsrnn_resampler_bank_create",
    "bsrnn_resample_len", "bsrnn_resampler_bank_create", "bsrnn_resampler_bank_assign", "bsrnn_resampler_bank_assign",
    "bsrnn_resampler_bank_process", "bsrnn_stream_process_hops", "bsrnn_resampler_bank_process", "bsrnn_stream_process_hops",
    "bsrnn_resampler_bank_process", "bsrnn_stream_process_hops", "bsrnn_resampler_bank_process", "bsrnn_stream_process_rows",
    "bsrnn_resample_len", "bsrnn_resampler_bank_flush_rows", "bsrnn_stream_process_hops", "bsrnn_resampler_bank_process",
    "bsrnn_resample_len", "bsrnn_resampler_bank_flush_rows", "bsrnn_stream_reset_rows", "bsrnn_stream_get_row",
    "bsrnn_stream_reset_rows", "bsrnn_stream_set_row", "bsrnn_resampler_bank_reset_rows", "bsrnn_resampler_bank_reset_rows",
]
NATIVE_RATE_POOL_CALLS = [
    "bsrnn_resample_len", "bsrnn_pool_create_rates", "bsrnn_pool_open_rate", "bsrnn_pool_open_rate",
    "bsrnn_pool_open_rate", "bsrnn_pool_ready", "bsrnn_pool_ready", "bsrnn_pool_ready",
    "bsrnn_pool_feed", "bsrnn_pool_ready", "bsrnn_pool_ready", "bsrnn_pool_ready",
    "bsrnn_pool_feed", "bsrnn_pool_ready", "bsrnn_pool_ready", "bsrnn_pool_ready",
    "bsrnn_pool_feed", "bsrnn_pool_ready", "bsrnn_pool_ready", "bsrnn_pool_feed",
    "bsrnn_pool_drain_len", "bsrnn_pool_drain", "bsrnn_pool_stream", "bsrnn_stream_get_row",
    "bsrnn_pool_get_pending", "bsrnn_pool_close", "bsrnn_pool_open_rate", "bsrnn_pool_stream",
    "bsrnn_stream_set_row", "bsrnn_pool_set_pending", "bsrnn_pool_close", "bsrnn_pool_close",
    "bsrnn_pool_close",
]


@pytest.fixture(scope="module")
def model(sd_default):
    return make_model(sd_default)


def refused(call, message, exc=ValueError):
    with pytest.raises(exc) as excinfo:
        call()
    assert type(excinfo.value) is exc and str(excinfo.value) == message, (str(excinfo.value), message)


def test_rows_calls_refuse_with_their_exact_text(model):
    from speechseparation_amd.bsrnn import StreamingSeparator
    st = StreamingSeparator(model, channels=2)
    nf = st.row_floats()
    hop = torch.zeros((2, HOP), device="cuda")
    two = torch.zeros((2, 2 * HOP))
    for name, call in (("process_rows", lambda w, mix=1.0: st.process_rows(w, None, mix)), ("process_hops", lambda w, mix=1.0: st.process_hops(w, [1, 1], mix))):
        refused(lambda: call(torch.zeros((3, HOP))), "%s: expected wave [2, L*1024], got (3, 1024)" % name)
        refused(lambda: call(torch.zeros(HOP)), "%s: expected wave [2, L*1024], got (1024,)" % name)
        refused(lambda: call("wave"), "%s: expected wave [2, L*1024], got str" % name)
        refused(lambda: call(torch.zeros((2, 700), device="cuda")), "%s: wave must hold whole hops of 1024 samples, got 700 samples per row" % name)
        refused(lambda: call(hop, torch.ones(3)), "%s: mix must be a float or a tensor [2], got (3,)" % name)
        refused(lambda: call(hop, torch.ones((2, 1))), "%s: mix must be a float or a tensor [2], got (2, 1)" % name)
        refused(lambda: call(hop, "wet"), "%s: mix must be a float or a tensor [2], got str" % name)
        refused(lambda: call(hop, True), "%s: mix must be a float or a tensor [2], got bool" % name)
        refused(lambda: call(hop, None), "%s: mix must be a float or a tensor [2], got NoneType" % name)
    refused(lambda: st.process_rows(hop, 5), "process_rows: active must be a sequence of 2 flags, got int")
    refused(lambda: st.process_rows(hop, [True]), "process_rows: 1 flags for 2 rows")
    refused(lambda: st.process_rows(hop, torch.ones(3)), "process_rows: 3 flags for 2 rows")
    refused(lambda: st.process_rows(hop, [True], "wet"), "process_rows: 1 flags for 2 rows")                      # (the flags before the mix)
    refused(lambda: st.process_rows(torch.zeros((2, 700)), 5), "process_rows: wave must hold whole hops of 1024 samples, got 700 samples per row")
    refused(lambda: st.process_hops(torch.zeros((2, 256 * HOP)), [1, 1]), "process_hops: 256 hops, a call takes at most 255")
    refused(lambda: st.process_hops(torch.zeros((2, 256 * HOP)), 5), "process_hops: 256 hops, a call takes at most 255")       # (before the counts)
    refused(lambda: st.process_hops(two, 5), "process_hops: hops must be a sequence of 2 ints, got int")
    refused(lambda: st.process_hops(two, [1]), "process_hops: 1 counts for 2 rows")
    refused(lambda: st.process_hops(two, torch.ones(3, dtype=torch.int64)), "process_hops: 3 counts for 2 rows")
    refused(lambda: st.process_hops(two, [1, 1.0]), "process_hops: the count of row 1 must be an int, got float")
    refused(lambda: st.process_hops(two, [True, 1]), "process_hops: the count of row 0 must be an int, got bool")
    refused(lambda: st.process_hops(two, [3, 1]), "process_hops: row 0 has 3 hops, outside [0, 2]")
    refused(lambda: st.process_hops(two, [2, -1]), "process_hops: row 1 has -1 hops, outside [0, 2]")
    refused(lambda: st.process_hops(two, [3, 1], "wet"), "process_hops: row 0 has 3 hops, outside [0, 2]")       # (the counts before the mix)
    refused(lambda: st.process_hops(torch.zeros((2, 0)), [1, 0]), "process_hops: row 0 has 1 hops, outside [0, 0]")
    for name, call in (("set_row", lambda r: st.set_row(r, torch.zeros(nf))), ("get_row", st.get_row), ("reset_rows", lambda r: st.reset_rows([0, r]))):
        refused(lambda: call("0"), "%s: row must be an int, got str" % name)
        refused(lambda: call(True), "%s: row must be an int, got bool" % name)
        refused(lambda: call(1.0), "%s: row must be an int, got float" % name)
        refused(lambda: call(2), "%s: row 2 is outside [0, 2)" % name)
        refused(lambda: call(-1), "%s: row -1 is outside [0, 2)" % name)
    refused(lambda: st.set_row(0, torch.zeros(5)), "set_row: blob must be a tensor [%d], got (5,)" % nf)
    refused(lambda: st.set_row(0, torch.zeros((1, nf))), "set_row: blob must be a tensor [%d], got (1, %d)" % (nf, nf))
    refused(lambda: st.set_row(0, "blob"), "set_row: blob must be a tensor [%d], got str" % nf)
    refused(lambda: st.set_row(2, "blob"), "set_row: row 2 is outside [0, 2)")                                      # (the row before the blob)
    refused(lambda: st.reset_rows(1), "reset_rows: rows must be a sequence of ints, got int")
    refused(lambda: st.reset_rows([]), "reset_rows: no rows")
    # none of it moved the stream: its rows are those of a fresh one
    fresh = StreamingSeparator(model, channels=2)
    assert all(torch.equal(st.get_row(r), fresh.get_row(r)) for r in range(2))
    assert st.process_rows(torch.zeros((2, 0))).shape == (2, 0) and st.process_hops(torch.zeros((2, 0)), [0, 0]).shape == (2, 0)


def test_resampler_bank_refuses_with_its_exact_text(model):
    from speechseparation_amd.bsrnn import ResamplerBank
    bank = ResamplerBank(model, 2, [(48000, 44100)])
    wave = torch.zeros((2, 100), device="cuda")
    refused(lambda: bank.process(torch.zeros((3, 100), device="cuda"), [1, 1]), "ResamplerBank.process: expected wave [C = 2, n], got (3, 100)")
    refused(lambda: bank.process("wave", [1, 1]), "ResamplerBank.process: expected wave [C = 2, n], got str")
    refused(lambda: bank.process(torch.zeros((2, 100)), [1, 1]), "ResamplerBank.process: expected a float32 tensor on %s, got torch.float32 on cpu" % bank.device)
    refused(lambda: bank.process(wave.double(), [1, 1]), "ResamplerBank.process: expected a float32 tensor on %s, got torch.float64 on %s" % (bank.device, wave.device))
    refused(lambda: bank.process(wave, 5), "ResamplerBank.process: counts must be a sequence of 2 ints, got int")
    refused(lambda: bank.process(wave, [1]), "ResamplerBank.process: 1 counts for 2 rows")
    refused(lambda: bank.process(wave, [1, 1.0]), "ResamplerBank.process: the count of row 1 must be an int, got float")
    refused(lambda: bank.process(wave, [101, 1]), "ResamplerBank.process: row 0 has 101 samples, outside [0, 100]")
    refused(lambda: bank.assign([0], 1), "ResamplerBank.assign: pair 1 is outside [0, 1)")
    refused(lambda: bank.assign(0, 0), "ResamplerBank.assign: rows must be a sequence of ints, got int")
    refused(lambda: bank.reset_rows([0, "1"]), "ResamplerBank.reset_rows: a row must be an int, got str")
    refused(lambda: bank.flush_rows([2]), "ResamplerBank.flush_rows: row 2 is outside [0, 2)")
    refused(lambda: bank.flush_rows([1, 1]), "ResamplerBank.flush_rows: a row is listed twice in [1, 1]")
    refused(lambda: bank.ready(True, 10), "ResamplerBank.ready: a row must be an int, got bool")
    refused(lambda: bank.pair_of(-1), "ResamplerBank.pair_of: row -1 is outside [0, 2)")
    assert bank.pair_of(1) == 0


class Recorder:
    """Stands in front of the library in the modules that hold the streaming classes and notes the name of every call."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def audio(n, seed):
    return 0.1 * torch.randn((1, n), generator=torch.Generator().manual_seed(seed)).cuda()


def script(pool):
    """One fixed life of a pool of 3 slots x 1 row with rates = (48000,)."""
    a, b, c = pool.open(sample_rate=48000), pool.open(), pool.open()
    sizes = (700, 1024, 2100)
    for tick in range(3):
        got = pool.feed({sid: audio(sizes[(k + tick) % 3], 10 * tick + k) for k, sid in enumerate((a, b, c))})
        assert sorted(got) == [a, b, c]
    got = pool.step({b: audio(HOP, 40), c: audio(HOP, 41)})
    assert got[b].shape == (1, HOP) and got[c].shape == (1, HOP)
    assert pool.drain(a).shape[0] == 1
    carry = pool.export(b)
    pool.close(b)
    d = pool.adopt(*carry) if isinstance(carry, tuple) else pool.adopt(carry)
    assert pool.sessions() == [a, c, d]
    for sid in (a, c, d):
        pool.close(sid)
    assert pool.sessions() == []


def recorded(model, monkeypatch, make):
    from speechseparation_amd import bsrnn
    from speechseparation_amd.bsrnn import NativeRatePool, ResamplerBank, StreamingSeparator, StreamPool
    StreamingSeparator(model, channels=2).step(torch.zeros((2, HOP), device="cuda"))       # (the model's weights are on the device)
    rec = Recorder(bsrnn._lib)
    for mod in {bsrnn} | {sys.modules[cls.__module__] for cls in (StreamingSeparator, ResamplerBank, StreamPool, NativeRatePool)}:
        monkeypatch.setattr(mod, "_lib", rec)
    script(make(model))
    monkeypatch.undo()
    names = [n for n in rec.names if not n.endswith("_destroy")]
    print("%d library calls:" % len(names))
    for i in range(0, len(names), 4):
        print("    " + "".join('"%s", ' % n for n in names[i:i + 4]).rstrip())
    return names


def test_stream_pool_makes_the_library_calls_it_made(model, monkeypatch):
    from speechseparation_amd.bsrnn import StreamPool
    assert recorded(model, monkeypatch, lambda m: StreamPool(m, 3, rates=(48000,))) == STREAM_POOL_CALLS


def test_native_rate_pool_makes_the_library_calls_it_made(model, monkeypatch):
    from speechseparation_amd.bsrnn import NativeRatePool
    assert recorded(model, monkeypatch, lambda m: NativeRatePool(m, 3, rates=(48000,))) == NATIVE_RATE_POOL_CALLS
