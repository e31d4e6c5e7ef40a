"""The overlapped dual path (csrc/api.hip::run_overlapped, kernels.h OvlProducer / OvlConsumer): the second band block runs beside the
first time-axis launch and the mask chain beside the second, on an auxiliary stream, each consumer workgroup waiting for the frames of
its own rows.  Same kernels and arithmetic as the serial flow, another dispatch order: every result must be EQUAL to BSRNN_OVERLAP=0,
call after call, also beside other work on the GPU; a consumer whose bounded wait expires is reported and the call falls back."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu


def make_model(sd, overlap, epochs=None):
    """A model whose context is created under BSRNN_OVERLAP=<overlap> (read once per context, csrc/api.hip::bsrnn_create)."""
    from speechseparation_amd.bsrnn import BSRNN
    old = os.environ.get("BSRNN_OVERLAP")
    if epochs is not None:
        os.environ["BSRNN_OVL_EPOCHS"] = str(epochs)
    if overlap is None:
        os.environ.pop("BSRNN_OVERLAP", None)
    else:
        os.environ["BSRNN_OVERLAP"] = overlap
    try:
        m = BSRNN().eval()
        m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}, strict=True)
        m = m.to("cuda")
        m._context(torch.device("cuda", torch.cuda.current_device()))
    finally:
        os.environ.pop("BSRNN_OVL_EPOCHS", None)
        if old is None:
            os.environ.pop("BSRNN_OVERLAP", None)
        else:
            os.environ["BSRNN_OVERLAP"] = old
    return m


@pytest.fixture(scope="module")
def models(sd_hot):
    return make_model(sd_hot, None), make_model(sd_hot, "0")


def test_overlapped_dual_path_equals_the_serial_flow_bit_for_bit(models):
    from speechseparation_amd import weights
    ovl, ser = models
    assert ovl.overlap_state() == 1 and ser.overlap_state() == 0
    # the metric's configuration (64 rows x 8 s @ 16 kHz: T = 126, 192 time-axis workgroups, 504 band tiles of which 63 straddle two rows)
    w = torch.from_numpy(weights.synth_waveform(64, 128000, seed=5)).cuda()
    ref = ser.separate(w).cpu().numpy()
    for i in range(6):
        assert np.array_equal(ovl.separate(w).cpu().numpy(), ref), "call %d" % i
    # the reference's operator (with the mask) on a ragged batch: 17 rows x 77 frames (51 time-axis workgroups, the last one ragged)
    x = ser.stft(torch.from_numpy(weights.synth_waveform(17, 76 * 1024 + 300, seed=6)).cuda())
    y0, m0 = ser.forward_with_mask(x)
    y1, m1 = ovl.forward_with_mask(x)
    assert torch.equal(y0, y1) and torch.equal(m0, m1)
    # a chunk with carried state (causal time axis): 16 rows x 64 frames
    xc = x[:16, :, :64].contiguous()
    s = torch.from_numpy(np.random.default_rng(3).standard_normal((4, 2, 16 * 12, 64)).astype(np.float32) * 0.3).cuda()
    z0, s0 = ser.forward_chunk(xc, s)
    z1, s1 = ovl.forward_chunk(xc, s)
    assert torch.equal(z0, z1) and torch.equal(s0, s1)
    assert ovl.overlap_state() == 1          # nothing gave up


def test_overlapped_results_do_not_depend_on_other_work_on_the_gpu(models):
    """Hand-offs inside a launch are to be tested under UNEVEN load with every word checked (cdna_hip_programming.md, Guideline 16):
    large matrix products on a second torch stream start and stop while the overlapped calls run."""
    from speechseparation_amd import weights
    ovl, ser = models
    w = torch.from_numpy(weights.synth_waveform(48, 100 * 1024 + 11, seed=7)).cuda()
    ref = ser.separate(w).cpu().numpy()
    a = torch.randn(4096, 4096, device="cuda")
    side = torch.cuda.Stream()
    outs = []
    for i in range(24):
        if i % 3 != 2:
            with torch.cuda.stream(side):
                for _ in range(1 + i % 4):
                    a = torch.tanh(a @ a * 1e-3)
        outs.append(ovl.separate(w))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert np.array_equal(o.cpu().numpy(), ref), "call %d" % i
    assert ovl.overlap_state() == 1


def test_a_consumer_that_gives_up_is_reported_and_the_call_falls_back(sd_hot):
    """BSRNN_OVERLAP=timeout (test hook): the time-axis launches publish no progress and the consumers' waits are cut to ~2 ms - every
    consumer workgroup gives up (guard value 5).  The call must notice, run again launch after launch and return the right numbers with
    rc 0; the context stays on the serial flow."""
    from speechseparation_amd import weights
    ser = make_model(sd_hot, "0")
    bad = make_model(sd_hot, "timeout")
    assert bad.overlap_state() == 1
    w = torch.from_numpy(weights.synth_waveform(16, 40 * 1024 + 5, seed=8)).cuda()
    ref = ser.separate(w).cpu().numpy()
    assert np.array_equal(bad.separate(w).cpu().numpy(), ref)
    assert bad.overlap_state() == 2
    assert np.array_equal(bad.separate(w).cpu().numpy(), ref)
    # under the 'deferred' policy nothing waits: the next call reports it (and that context stops overlapping, too)
    from speechseparation_amd._native import NativeError
    bad2 = make_model(sd_hot, "timeout")
    bad2.set_range_policy("deferred")
    bad2.separate(w)
    torch.cuda.synchronize()
    with pytest.raises(NativeError):
        bad2.separate(w)
    assert bad2.overlap_state() == 2
    assert np.array_equal(bad2.separate(w).cpu().numpy(), ref)


def test_batches_in_flight_on_contexts_of_their_own_equal_one_after_the_other(sd_hot):
    """Two and three independent contexts, each on a stream of its own, `separate()` calls alternating without a host wait between them
    (bench.py's `batches_in_flight`; how a server with several request queues drives the C ABI): every kernel of one batch then runs beside
    kernels of another - the overlapped dual path's progress words, gates and auxiliary streams included, all of which are per context.
    Every output equals the same call made alone."""
    from speechseparation_amd import weights
    ctxs = [make_model(sd_hot, None) for _ in range(3)]
    streams = [torch.cuda.Stream() for _ in range(3)]
    waves = [torch.from_numpy(weights.synth_waveform(64, 128000, seed=40 + j)).cuda() for j in range(3)]
    refs = [ctxs[0].separate(w).clone() for w in waves]            # one context, one stream, one call at a time
    torch.cuda.synchronize()
    for m in ctxs:
        m.set_range_policy("deferred")
    outs = [torch.empty_like(refs[0]) for _ in range(3)]
    for n in (2, 3):
        for rep in range(8):
            for j in range(n):
                with torch.cuda.stream(streams[j]):
                    ctxs[j].separate(waves[j], out=outs[j])
            if rep % 4 == 3:
                torch.cuda.synchronize()
                for j in range(n):
                    assert torch.equal(outs[j], refs[j]), "contexts in flight %d, round %d, context %d" % (n, rep, j)
                    outs[j].zero_()
    for j, m in enumerate(ctxs):
        with torch.cuda.stream(streams[j]):
            m.sync()                                                  # (raises on a guard word left set)
        assert m.overlap_state() == 1


def test_progress_word_epochs_start_again(sd_hot, models):
    """The progress words carry the call's number on the context in their upper bits and start again every 2^18 calls (device idle, words
    zeroed).  With the period set to 5 calls (test hook BSRNN_OVL_EPOCHS) the restart happens every few calls, between calls of two shapes:
    every result equals the serial flow."""
    from speechseparation_amd import weights
    _, ser = models
    m = make_model(sd_hot, None, epochs=5)
    m.set_range_policy("deferred")
    shapes = [(64, 128000, 7), (20, 70 * 1024 + 100, 8)]
    waves = [torch.from_numpy(weights.synth_waveform(r, n, seed=sd)).cuda() for r, n, sd in shapes]
    refs = [ser.separate(w).clone() for w in waves]
    for i in range(23):
        k = i % 2
        assert torch.equal(m.separate(waves[k]), refs[k]), "call %d" % i
    m.sync()
    assert m.overlap_state() == 1


def test_a_batch_whose_time_axis_launch_takes_eight_sequences_per_workgroup_overlaps_too(models):
    """100 rows x 12 bands = 1 200 sequences: four per workgroup would be 300 workgroups (more than one per CU), so the time-axis launches run
    eight per workgroup (plan_host.h::plan_call, Flow::seqs) - 150 workgroups, inside the overlap's range: the consumers then map sequences to producer
    workgroups eight at a time (OvlConsumer::wg_shift).  Equal to the serial flow."""
    from speechseparation_amd import weights
    ovl, ser = models
    w = torch.from_numpy(weights.synth_waveform(100, 48 * 1024 + 11, seed=9)).cuda()
    ref = ser.separate(w).cpu().numpy()
    for i in range(3):
        assert np.array_equal(ovl.separate(w).cpu().numpy(), ref), "call %d" % i
    assert ovl.overlap_state() == 1


_EVAL_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, %r)
from speechseparation_amd import weights
from speechseparation_amd.bsrnn import BSRNN
sd = weights.synth_state_dict(None, seed=1, lstm_gain=3.0)
def model(overlap):
    os.environ["BSRNN_OVERLAP"] = overlap                # (read when the context is created)
    m = BSRNN().eval(); m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}, strict=True); m = m.to("cuda")
    m._context(torch.device("cuda", torch.cuda.current_device()))
    return m
ser, bad = model("0"), model("timeout")
bad.set_range_policy("deferred")
w = weights.synth_waveform(16, 40 * 1024 + 5, seed=8)
mix, speech = torch.from_numpy(w).cuda(), torch.from_numpy(0.5 * w + 0.1 * weights.synth_waveform(16, 40 * 1024 + 5, seed=9)).cuda()
ref = ser.evaluate(mix, speech)
assert bad.overlap_state() == 1
for i in range(2):
    got = bad.evaluate(mix, speech)
    assert got == ref, (i, got, ref)
    print("call", i, "overlap_state", bad.overlap_state())
bad.sync()
print("EVAL OK overlap_state", bad.overlap_state())
"""


def test_evaluate_falls_back_from_an_expired_wait_under_the_deferred_policy():
    """evaluate() is synchronous: whatever the range policy, it ends like a call under the default policy.  16 rows x 41 frames (48 time-axis
    workgroups, one row block: the overlapped path) under BSRNN_OVERLAP=timeout (test hook: every consumer gives up, guard value 5) and the
    'deferred' policy: rc 0, the metrics of the serial flow exactly, and the context stops overlapping (overlap_state 2).  In a child process
    of its own (knobs are read once)."""
    r = subprocess.run([sys.executable, "-c", _EVAL_SCRIPT % REPO], env=dict(os.environ), cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "call 0 overlap_state 2" in r.stdout and "EVAL OK overlap_state 2" in r.stdout, r.stdout[-3000:]
