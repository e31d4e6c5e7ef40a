"""GPU: the ragged long-form evaluate (BSRNN.evaluate_long_ragged -> bsrnn_evaluate_long_ragged, BSRNN.evaluate_long / evaluate_many_long,
validate.py --segment-frames): the reference's validation metrics PER CLIP for clips of different lengths, with the separation cut into
segments and every sum formed segment by segment.  Expected values are the oracle's stock-PyTorch restatement
(oracle/metrics_torch.train_infer) on each clip's own samples; the comparisons of the library with itself are the ones the interface
promises.

Signals and bounds are those of tests/test_gpu_evaluate_ragged.py: speech = synth_waveform(seed 612, 0.07), mix = speech +
synth_waveform(seed 611, 0.05); 2e-3 dB on the four decibel figures, 2e-5 relative on the L1 terms and the loss, 1e-4 max-abs on the
estimate against the oracle, 3e-5 against `separate` / `evaluate` of the clip alone.  Those bounds already leave room for an estimate
that moves by 3e-5 (that file's docstring), which is what a segmented separation does to it.

Shapes: five clips of 2, 1, 2, 2, 3 rows with 10, 4, 5, 8, 2 frames, an odd stride (scalar loads), in that order - which has ended clips
inside the alive prefix - and longest first; segments of 1 frame (the first completes no hop, every later one exactly one), 3 and 4 frames
(a row ends inside a segment, exactly at an edge - 4 frames at 4 per segment - and one frame past an edge - 4 frames at 3, 5 frames at 4).
One length is a multiple of 1024.  The equal-length test takes the 16-byte loads.

What the coarse bounds cannot see - a hop counted twice or not at all moves a figure by less than 2e-3 dB when the clip is long - the
time-domain test sees: the figures recomputed in numpy from the RETURNED estimate agree to 1e-5 dB / 1e-9 relative, the bounds
test_equal_lengths_are_evaluate holds for double sums in another order."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu
DB_TOL, REL_TOL, EST_TOL, TOL_VS_SEPARATE = 2e-3, 2e-5, 1e-4, 3e-5
KEYS = ("loss", "sdr", "input_sdr", "sisdr", "l1_time", "l1_re", "l1_im", "separation_db")
DB_KEYS = ("sdr", "input_sdr", "sisdr", "separation_db")
LENS = [9 * 1024 + 77, 3 * 1024 + 5, 4 * 1024, 7 * 1024 + 1023, 1500]
ROWS = [2, 1, 2, 2, 3]
FIRST = [0, 2, 3, 5, 7]
STRIDE = 9 * 1024 + 77
ORDERS = {"given": [0, 1, 2, 3, 4], "longest_first": [0, 3, 2, 1, 4]}
SEGS = (1, 3, 4)


def kept(n):
    return (n // 1024) * 1024


def make_model(sd):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}, strict=True)
    return m.to("cuda")


def make_oracle(sd):
    from oracle.bsrnn_torch_cpu import TorchCpuBSRNN
    from speechseparation_amd import spec
    return TorchCpuBSRNN(sd, spec.generate_bandsplits()[0])


def signals(rows, n, row_offset=0):
    from speechseparation_amd import weights
    speech = weights.synth_waveform(rows, n, seed=612, scale=0.07, row_offset=row_offset)
    mix = speech + weights.synth_waveform(rows, n, seed=611, scale=0.05, row_offset=row_offset)
    return mix.astype(np.float32), speech


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def counter(which):
    from speechseparation_amd import _native
    return _native.lib.bsrnn_debug_counter(which)


def ordered(mix, speech, order):
    """The batch with its clips in another order: (mix, speech, lens, rows)."""
    pick = np.concatenate([np.arange(FIRST[c], FIRST[c] + ROWS[c]) for c in order])
    return mix[pick], speech[pick], [LENS[c] for c in order], [ROWS[c] for c in order]


def row_frames(lens, rows):
    from speechseparation_amd import spec
    return [spec.n_frames(n) for n, ch in zip(lens, rows) for _ in range(ch)]


def compare(got, ref, what, db_tol=DB_TOL, rel_tol=REL_TOL):
    """Every figure printed, then held to its bound: absolute on the decibel figures, relative on the L1 terms and the loss."""
    bad = []
    for k in KEYS:
        d = abs(got[k] - ref[k])
        if k in DB_KEYS:
            print("%s %-13s got %+.6f ref %+.6f diff %.2e dB (bound %.0e)" % (what, k, got[k], ref[k], d, db_tol))
            ok = d < db_tol
        else:
            print("%s %-13s got %.8e ref %.8e rel %.2e (bound %.0e)" % (what, k, got[k], ref[k], d / abs(ref[k]), rel_tol))
            ok = d <= rel_tol * abs(ref[k])
        if not ok or not np.isfinite(got[k]):
            bad.append((k, got[k], ref[k]))
    assert not bad, (what, bad)


def numbers(results):
    return [[d[k] for k in KEYS] for d in results]


@pytest.fixture(scope="module")
def model(sd_default):
    return make_model(sd_default)


@pytest.fixture(scope="module")
def batch(sd_default):
    """(mix, speech [10, STRIDE], the oracle's metrics and estimate of every clip on its own samples), computed once, left unchanged."""
    from oracle import metrics_torch as mt
    oracle = make_oracle(sd_default)
    mix, speech = signals(sum(ROWS), STRIDE)
    refs = []
    for r0, ch, n in zip(FIRST, ROWS, LENS):
        refs.append(mt.train_infer(oracle.forward, torch.from_numpy(mix[r0:r0 + ch, :n].copy()), torch.from_numpy(speech[r0:r0 + ch, :n].copy())))
    mix.setflags(write=False)
    speech.setflags(write=False)
    return mix, speech, refs


@pytest.fixture(scope="module")
def singles(model, batch):
    """`evaluate` of every clip alone, with its estimate; computed once."""
    mix, speech, _ = batch
    return [model.evaluate(dev(mix[r0:r0 + ch, :n]), dev(speech[r0:r0 + ch, :n]), return_estimate=True) for r0, ch, n in zip(FIRST, ROWS, LENS)]


@pytest.fixture(scope="module")
def segmented(model, batch):
    """The call on the batch in both orders at every segment length, with the estimates; computed once, shared."""
    mix, speech, _ = batch
    out = {}
    for name, order in ORDERS.items():
        m, s, lens, rows = ordered(mix, speech, order)
        for seg in SEGS:
            out[name, seg] = model.evaluate_long_ragged(dev(m), dev(s), lens, rows, seg, return_estimate=True)
    return out


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_per_clip_against_the_oracle_and_evaluate_alone(batch, singles, segmented, order, seg):
    _, _, refs = batch
    got_all = segmented[order, seg]
    assert len(got_all) == 5
    for got, c in zip(got_all, ORDERS[order]):
        ref, one = refs[c], singles[c]
        assert set(got) == set(KEYS) | {"x_time"}
        x = got["x_time"]
        assert tuple(x.shape) == (ROWS[c], kept(LENS[c])) == tuple(ref["x_time"].shape) and x.is_cuda and x.dtype == torch.float32
        e = float((x.cpu() - ref["x_time"]).abs().max())
        e1 = float((x - one["x_time"]).abs().max())
        print("%s seg %d clip %d: max|est - oracle| %.3e  max|est - evaluate est| %.3e" % (order, seg, c, e, e1))
        assert e < EST_TOL, (c, e)
        assert e1 < TOL_VS_SEPARATE, (c, e1)
        compare(got, ref, "%s seg %d clip %d vs oracle:" % (order, seg, c))
        compare(got, one, "%s seg %d clip %d vs evaluate alone:" % (order, seg, c))
        # whatever the kernels do: a mean of |x - s| moves by at most the largest change of x
        assert abs(got["l1_time"] - ref["l1_time"]) <= e + REL_TOL * ref["l1_time"], (c, got["l1_time"], ref["l1_time"], e)


@pytest.mark.parametrize("seg", SEGS)
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_time_domain_figures_from_the_returned_estimate(batch, segmented, order, seg):
    """sdr, sisdr, l1_time and separation_db recomputed from the returned x_time by the documented arithmetic - fp32 differences, float64
    sums, alpha in fp32, the SI-SDR by its two passes - agree to 1e-5 dB and 1e-9 relative: every hop of every row was counted once."""
    mix, speech, _ = batch
    eps = np.float32(1.1920928955078125e-07)
    for got, c in zip(segmented[order, seg], ORDERS[order]):
        r0, ch, n = FIRST[c], ROWS[c], LENS[c]
        x = got["x_time"].cpu().numpy()
        s, m = speech[r0:r0 + ch, :kept(n)], mix[r0:r0 + ch, :kept(n)]
        assert x.dtype == np.float32 and s.dtype == np.float32 and m.dtype == np.float32
        d, b = x - s, m - x                                                    # fp32 differences
        f8 = np.float64
        ss, dd, xs = (s.astype(f8) ** 2).sum(1), (d.astype(f8) ** 2).sum(1), (x.astype(f8) * s.astype(f8)).sum(1)
        sdr = float(np.mean(10.0 * np.log10((ss + 1e-9) / (dd + 1e-9))))
        alpha = ((xs.astype(np.float32) + eps) / (ss.astype(np.float32) + eps)).astype(np.float32)
        ts = alpha[:, None] * s
        nz = ts - x
        sisdr = float(np.mean(10.0 * np.log10(((ts.astype(f8) ** 2).sum(1) + f8(eps)) / ((nz.astype(f8) ** 2).sum(1) + f8(eps)))))
        l1 = float(np.abs(d).astype(f8).sum() / (ch * kept(n)))
        sep = float(10.0 * np.log((m.astype(f8) ** 2).sum() / (b.astype(f8) ** 2).sum()))
        for k, v in (("sdr", sdr), ("sisdr", sisdr), ("separation_db", sep)):
            print("%s seg %d clip %d %-13s library %+.9f numpy %+.9f diff %.2e dB" % (order, seg, c, k, got[k], v, abs(got[k] - v)))
        print("%s seg %d clip %d l1_time       library %.12e numpy %.12e rel %.2e" % (order, seg, c, got["l1_time"], l1, abs(got["l1_time"] - l1) / l1))
        for k, v in (("sdr", sdr), ("sisdr", sisdr), ("separation_db", sep)):
            assert abs(got[k] - v) < 1e-5, (c, k, got[k], v)
        assert abs(got["l1_time"] - l1) <= 1e-9 * l1, (c, got["l1_time"], l1)


def test_one_segment_is_evaluate_ragged(model, batch):
    mix, speech, _ = batch
    wm, ws = dev(mix), dev(speech)
    rag = model.evaluate_ragged(wm, ws, LENS, ROWS, return_estimate=True)
    for seg in (10, 256):
        got = model.evaluate_long_ragged(wm, ws, LENS, ROWS, seg, return_estimate=True)
        assert numbers(got) == numbers(rag), seg
        for c in range(5):
            assert torch.equal(got[c]["x_time"], rag[c]["x_time"]), (seg, c)
        assert numbers(model.evaluate_long_ragged(wm, ws, LENS, ROWS, seg)) == numbers(rag), seg


@pytest.mark.parametrize("extra", [0, 3])
def test_equal_lengths(model, extra):
    """One clip of 3 rows of 16384 samples in segments of 4 frames: the estimate is `separate_long`'s bit for bit, the metrics are within the
    bounds of `evaluate`; `evaluate_long` is the same call.  extra = 0: rows 16-byte aligned, the time kernel's 16-byte loads; extra = 3: a
    stride of n + 3, its scalar loads - the same samples, so the same sums to the order of the double additions."""
    n = 16384
    mix, speech = signals(3, n)
    one = model.evaluate(dev(mix), dev(speech), return_estimate=True)
    long_est = model.separate_long(dev(mix), 4)
    wm, ws = np.zeros((3, n + extra), np.float32), np.zeros((3, n + extra), np.float32)
    wm[:, :n], ws[:, :n] = mix, speech
    got = model.evaluate_long_ragged(dev(wm), dev(ws), [n], [3], 4, return_estimate=True)
    assert len(got) == 1
    assert torch.equal(got[0]["x_time"], long_est)
    compare(got[0], one, "stride n + %d vs evaluate:" % extra)
    if extra == 0:
        whole = model.evaluate_long(dev(mix), dev(speech), 4, return_estimate=True)
        assert torch.equal(whole["x_time"], long_est)
        assert [whole[k] for k in KEYS] == [got[0][k] for k in KEYS]
    else:
        aligned = model.evaluate_long_ragged(dev(mix), dev(speech), [n], [3], 4)
        for k in KEYS:
            d = abs(got[0][k] - aligned[0][k])
            print("%-13s scalar loads %.12e 16-byte loads %.12e diff %.2e" % (k, got[0][k], aligned[0][k], d))
            assert d < 1e-5 if k in DB_KEYS else d <= 1e-9 * abs(aligned[0][k]), (k, got[0][k], aligned[0][k])


@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_nothing_behind_a_clips_end_is_read_nothing_stale_is_used(sd_default, batch, fill):
    """Behind every clip's end both inputs hold NaN / 1e30; the workspace (a one-shot call on NaN) and the long-form carry sets (a segmented
    call on NaN) hold NaN beforehand.  Numbers and estimates have the bits of a fresh context's call on the clean inputs."""
    mix, speech, _ = batch
    fresh = make_model(sd_default)
    expect = fresh.evaluate_long_ragged(dev(mix), dev(speech), LENS, ROWS, 3, return_estimate=True)
    m = make_model(sd_default)
    nan_in = torch.full((12, STRIDE + 2048), float("nan"), device="cuda")
    assert torch.isnan(m.separate(nan_in)).all()                              # NaN all over a larger workspace
    assert torch.isnan(m.separate_long(nan_in, 3)).all()                      # ... and in both sets of LSTM state and overlap-add tail
    dm, ds = np.array(mix), np.array(speech)
    for r0, ch, n in zip(FIRST, ROWS, LENS):
        dm[r0:r0 + ch, n:] = fill
        ds[r0:r0 + ch, n:] = fill
    got = m.evaluate_long_ragged(dev(dm), dev(ds), LENS, ROWS, 3, return_estimate=True)
    a, b = np.array(numbers(got)), np.array(numbers(expect))
    print("tails %r, dirty workspace and carry: largest |difference| of the 40 numbers to a fresh context %.3e" % (fill, np.abs(a - b).max()))
    assert a.shape == (5, 8) and np.isfinite(a).all()
    assert (a == b).all(), (a - b)
    for c in range(5):
        assert torch.equal(got[c]["x_time"], expect[c]["x_time"]), c
    # without an estimate the segment buffer takes its place: the same numbers
    again = m.evaluate_long_ragged(dev(dm), dev(ds), LENS, ROWS, 3)
    assert numbers(again) == numbers(expect)


def test_run_equals_rerun_and_a_second_call_allocates_nothing(sd_default, batch, segmented):
    mix, speech, _ = batch
    m = make_model(sd_default)
    wm, ws = dev(mix), dev(speech)
    for estimate in (True, False):
        first = m.evaluate_long_ragged(wm, ws, LENS, ROWS, 3, return_estimate=estimate)
        rows, allocs = m.workspace_rows(), counter(0)
        second = m.evaluate_long_ragged(wm, ws, LENS, ROWS, 3, return_estimate=estimate)
        assert (m.workspace_rows(), counter(0)) == (rows, allocs)
        assert numbers(second) == numbers(first) == numbers(segmented["given", 3])       # bit for bit: a fixed order of additions
        assert all(("x_time" in d) == estimate for d in second)
        if estimate:
            for a, b in zip(first, second):
                assert torch.equal(a["x_time"], b["x_time"])


@pytest.mark.parametrize("order,seg", [("longest_first", 3), ("longest_first", 1), ("given", 3), ("given", 4)])
def test_rows_retire(sd_default, batch, segmented, order, seg):
    """The frame rows handed to the model are the plan's (bsrnn_debug_counter(4)), below the rectangle's 100 when rows retire - 56 of them are real -, and the
    workspace of a fresh context is that of one segment."""
    from speechseparation_amd import spec
    mix, speech, _ = batch
    m_, s_, lens, rows = ordered(mix, speech, ORDERS[order])
    frames = row_frames(lens, rows)
    _, total = spec.long_plan(frames, seg)
    assert sum(frames) == 56 <= total < 10 * 10
    m = make_model(sd_default)
    assert m.workspace_rows() == 0
    before = counter(4)
    got = m.evaluate_long_ragged(dev(m_), dev(s_), lens, rows, seg)
    assert counter(4) - before == total
    assert 0 < m.workspace_rows() <= 10 * seg
    assert numbers(got) == numbers(segmented[order, seg])


def test_range_policy_per_segment(model, batch):
    """Samples 3*1024 .. 5*1024 - 1 of the first clip's mixture reach its frames 3, 4 and 5 only: with three frames per segment exactly the
    second segment.  Scaled by 3e5 they drive that clip's spectrum beyond the fp16x2 operand range: the segment is run again on the
    exact-fp32 kernels, its sums are added once, the call returns rc 0 with every number finite and the other clips within the bounds of
    their oracle.  For the scaled clip itself no bound can be derived here (its estimate is far from its target).  Then: nothing is left
    pending, and an in-range call under the `deferred` policy gives the numbers of `exact` - the guard is handled per segment either way."""
    mix, speech, refs = batch
    ws = dev(speech)
    big = np.array(mix, np.float64)
    big[0:2, 3 * 1024:5 * 1024] *= 3e5
    big = big.astype(np.float32)
    got = model.evaluate_long_ragged(dev(big), ws, LENS, ROWS, 3, return_estimate=True)      # (a non-zero rc raises NativeError)
    a = np.array(numbers(got))
    assert np.isfinite(a).all(), a
    assert torch.isfinite(got[0]["x_time"]).all()
    for c in (1, 2, 3, 4):
        e = float((got[c]["x_time"].cpu() - refs[c]["x_time"]).abs().max())
        print("clip %d beside the scaled one: max|est - oracle| %.3e" % (c, e))
        assert e < EST_TOL
        compare(got[c], refs[c], "clip %d beside the scaled one vs oracle:" % c)
    exact = model.evaluate_long_ragged(dev(mix), ws, LENS, ROWS, 3, return_estimate=True)
    model.set_range_policy("deferred")
    try:
        deferred = model.evaluate_long_ragged(dev(mix), ws, LENS, ROWS, 3, return_estimate=True)
        scaled = model.evaluate_long_ragged(dev(big), ws, LENS, ROWS, 3)
        model.sync()
    finally:
        model.set_range_policy("exact")
    assert numbers(deferred) == numbers(exact)
    for c in range(5):
        assert torch.equal(deferred[c]["x_time"], exact[c]["x_time"]), c
    assert numbers(scaled) == numbers(got)                                                   # the re-run happens under either policy
    for c in range(5):
        compare(exact[c], refs[c], "after the re-run, clip %d vs oracle:" % c)


def test_high_sdr_regime(sd_hot):
    """Targets close to the model's own output (SDR ~ 40 dB, where the noise sums are small differences and the SI-SDR's noise power is a
    cancellation of the row's totals): two clips of 12 and 5 frames in segments of 4.  Bounds of
    tests/test_gpu_evaluate_ragged.py::test_high_sdr_regime: 5e-3 dB, 5e-5."""
    from oracle import metrics_torch as mt
    from speechseparation_amd import weights
    model, oracle = make_model(sd_hot), make_oracle(sd_hot)
    lens, rows = [11 * 1024 + 300, 4 * 1024 + 9], [2, 1]
    mix = weights.synth_waveform(3, lens[0], seed=7)
    speech = np.zeros_like(mix)
    refs, r0 = [], 0
    for ch, n in zip(rows, lens):
        m = torch.from_numpy(mix[r0:r0 + ch, :n].copy())
        x_ref = oracle.separate(m)
        s = torch.zeros_like(m)
        s[:, :x_ref.shape[1]] = x_ref + 0.01 * x_ref.abs().max() * torch.from_numpy(
            weights.synth_waveform(ch, x_ref.shape[1], seed=8, scale=1.0, row_offset=r0))
        speech[r0:r0 + ch, :n] = s.numpy()
        refs.append(mt.train_infer(oracle.forward, m, s))
        r0 += ch
    got = model.evaluate_long_ragged(dev(mix), dev(speech), lens, rows, 4)
    for c, (g, ref) in enumerate(zip(got, refs)):
        assert ref["sdr"] > 20, ref["sdr"]
        compare(g, ref, "high SDR, clip %d vs oracle:" % c, db_tol=5e-3, rel_tol=5e-5)


def test_evaluate_many_long(model, batch):
    """The five pairs and a mono pair (clip 1's signals as 1-D tensors), some on the CPU; max_rows = 4 makes several buckets."""
    from speechseparation_amd import metrics, spec
    mix, speech, refs = batch
    pairs, expect = [], []
    for c, (r0, ch, n) in enumerate(zip(FIRST, ROWS, LENS)):
        p = (torch.from_numpy(mix[r0:r0 + ch, :n].copy()), torch.from_numpy(speech[r0:r0 + ch, :n + (5 if c == 3 else 0)].copy()))
        pairs.append(p if c in (1, 3) else tuple(t.cuda() for t in p))         # (pair 3's clean signal is longer: cut to the common length)
        expect.append(refs[c])
    pairs.append((torch.from_numpy(mix[2, :LENS[1]].copy()).cuda(), torch.from_numpy(speech[2, :LENS[1]].copy())))
    expect.append(refs[1])
    buckets = spec.long_buckets([1 + n // 1024 for n in LENS + [LENS[1]]], ROWS + [1], 4)
    assert len(buckets) >= 3 and sorted(i for b in buckets for i in b) == list(range(6))
    outs = metrics.evaluate_many_long(model, pairs, segment_frames=3, max_rows=4)
    assert len(outs) == 6
    for i, (got, ref) in enumerate(zip(outs, expect)):
        assert set(got) == set(KEYS)
        compare(got, ref, "evaluate_many_long pair %d vs oracle:" % i)
    again = model.evaluate_many_long(pairs, 3, 4)
    assert numbers(again) == numbers(outs)


def test_validate_segment_frames(tmp_path):
    """validate.py --segment-frames 3 --batch-rows 8 on three stereo file pairs of different lengths prints the two lines of the default
    invocation."""
    from speechseparation_amd import audio
    files = []
    for i, n in enumerate((9000, 5000 + 13, 3 * 1024)):
        mix, speech = signals(2, n, row_offset=20 + 2 * i)
        pm, ps = str(tmp_path / ("mix%d.wav" % i)), str(tmp_path / ("speech%d.wav" % i))
        audio.save_wav(pm, torch.from_numpy(mix), 16000)
        audio.save_wav(ps, torch.from_numpy(speech), 16000)
        files += [pm, ps]

    def run(extra):
        out = subprocess.run([sys.executable, os.path.join(REPO, "validate.py"), "--pairs"] + files + ["--synthetic-weights", "0"] + extra,
                             capture_output=True, text=True, timeout=300, cwd=REPO)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.strip().splitlines()
        assert len(lines) == 2 and lines[0].startswith("Validation Loss") and lines[1].startswith("Validation input SDR"), out.stdout
        w = out.stdout.split()
        return {"loss": float(w[w.index("Loss") + 1]), "sdr": float(w[w.index("SDR") + 1]),
                "input_sdr": float(w[w.index("input") + 2]), "sisdr": float(w[w.index("SI-SDR") + 1])}
    default, long_form = run([]), run(["--segment-frames", "3", "--batch-rows", "8"])
    for k in ("loss", "sdr", "input_sdr", "sisdr"):
        print("validate.py %-9s default %.8f --segment-frames 3 --batch-rows 8 %.8f" % (k, default[k], long_form[k]))
    assert abs(long_form["loss"] - default["loss"]) <= REL_TOL * abs(default["loss"])
    for k in ("sdr", "input_sdr", "sisdr"):
        assert abs(long_form[k] - default[k]) < DB_TOL, (k, long_form[k], default[k])
