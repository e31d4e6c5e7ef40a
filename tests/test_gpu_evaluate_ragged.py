"""GPU: the ragged evaluate (BSRNN.evaluate_ragged -> bsrnn_evaluate_ragged, BSRNN.evaluate_many, validate.py --batch-rows): the
reference's validation metrics PER CLIP for a batch of clips of different lengths.  Expected values are the oracle's stock-PyTorch
restatement (oracle/metrics_torch.train_infer) on each clip's own samples; the comparisons of the library with itself are the ones the
interface promises (each clip as `evaluate` gives it alone, nothing behind a clip's end is read, a dirty workspace changes nothing, run ==
re-run bit for bit).

Bounds: those of tests/test_gpu_metrics.py - 2e-3 dB on the four decibel figures (the reference sums in fp32, the device in double), 2e-5
relative on the L1 terms and the loss - and 1e-4 max-abs on the estimate (the project's waveform contract).

Shapes: five clips of 2, 1, 2, 2, 3 rows and T_c = 10, 4, 5, 8, 2 frames, R = 10.  The DSP kernels walk 4 frames / hops per workgroup at
this size, so row ends fall inside a chunk, on a chunk boundary and one past it; one length is a multiple of 1024; the stride is odd, so
rows are not 16-byte aligned and the time kernel takes its scalar loads (the equal-length test takes the 16-byte ones).  The shortest
clip has 1500 samples, not the two-frame minimum of 1025: at 1025 both frames are symmetric about their centres and L1_IM is pure
rounding noise, which no relative bound describes.

Signals: speech = synth_waveform(seed 612, scale 0.07), mix = speech + synth_waveform(seed 611, scale 0.05).  With an independent target
SI-SDR sits near -40 dB, where an estimate difference of 3e-5 moves it by up to 3e-2 dB; with this correlated pair the oracle gives SDR
~ 1.1 dB, SI-SDR ~ -3.8 dB and INPUT_SDR ~ 3 dB for every clip, and +-3e-5 on every sample of the estimate (the project's bound between
kernel choices) moves SDR by <= 1.4e-4 dB and SI-SDR by <= 1.2e-3 dB: the bounds above keep their room."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu
DB_TOL, REL_TOL, EST_TOL = 2e-3, 2e-5, 1e-4
KEYS = ("loss", "sdr", "input_sdr", "sisdr", "l1_time", "l1_re", "l1_im", "separation_db")
DB_KEYS = ("sdr", "input_sdr", "sisdr", "separation_db")
LENS = [9 * 1024 + 77, 3 * 1024 + 5, 4 * 1024, 7 * 1024 + 1023, 1500]
ROWS = [2, 1, 2, 2, 3]
FIRST = [0, 2, 3, 5, 7]
STRIDE = 9 * 1024 + 77
EARG = 1


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
def clean(model, batch):
    """The ragged call on the batch as given, with its estimates; shared by the tests that compare with it."""
    mix, speech, _ = batch
    return model.evaluate_ragged(dev(mix), dev(speech), LENS, ROWS, return_estimate=True)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


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


def test_per_clip_against_the_oracle(batch, clean):
    _, _, refs = batch
    assert len(clean) == 5
    for c, (got, ref) in enumerate(zip(clean, refs)):
        assert set(got) == set(KEYS) | {"x_time"}
        x = got["x_time"]
        assert tuple(x.shape) == (ROWS[c], kept(LENS[c])) == tuple(ref["x_time"].shape) and x.is_cuda and x.dtype == torch.float32
        e = float((x.cpu() - ref["x_time"]).abs().max())
        print("clip %d: max|est - oracle| %.3e" % (c, e))
        assert e < EST_TOL, (c, e)
        compare(got, ref, "clip %d vs oracle:" % c)
        # whatever the kernels do: a mean of |x - s| moves by at most the largest change of x
        assert abs(got["l1_time"] - ref["l1_time"]) <= e + REL_TOL * ref["l1_time"], (c, got["l1_time"], ref["l1_time"], e)


def test_per_clip_against_evaluate_alone(model, batch, clean):
    mix, speech, _ = batch
    for c, (r0, ch, n) in enumerate(zip(FIRST, ROWS, LENS)):
        one = model.evaluate(dev(mix[r0:r0 + ch, :n]), dev(speech[r0:r0 + ch, :n]), return_estimate=True)
        e = float((clean[c]["x_time"] - one["x_time"]).abs().max())
        print("clip %d: max|ragged est - evaluate est| %.3e" % (c, e))
        assert e < 3e-5, (c, e)
        compare(clean[c], one, "clip %d vs evaluate alone:" % c)


@pytest.mark.parametrize("extra", [0, 3])
def test_equal_lengths_are_evaluate(model, extra):
    """One clip of 3 rows: the estimate is bit-identical to `evaluate`'s.  extra = 0: rows 16-byte aligned, and `evaluate` IS this batch -
    the same metric launches on the same grids, the same host tail - so the five figures that come from the waveforms alone are EQUAL; the
    spectral terms (and the loss that holds them) keep their bounds, because the clean signal goes through the rectangular analysis in
    one call and the ragged analysis in the other.  extra = 3: a stride of n + 3, the time kernel's scalar loads against 16-byte ones, so
    the metrics differ by the order of the double additions (sums of fewer than 1e5 non-negative doubles reorder within N * 2^-53) and at
    most one fp32 ulp of alpha."""
    n = 16384
    mix, speech = signals(3, n)
    one = model.evaluate(dev(mix), dev(speech), return_estimate=True)
    wm, ws = np.zeros((3, n + extra), np.float32), np.zeros((3, n + extra), np.float32)
    wm[:, :n], ws[:, :n] = mix, speech
    got = model.evaluate_ragged(dev(wm), dev(ws), [n], [3], return_estimate=True)
    assert len(got) == 1
    assert torch.equal(got[0]["x_time"], one["x_time"])
    for k in KEYS:
        d = abs(got[0][k] - one[k])
        print("stride n + %d %-13s ragged %.12e evaluate %.12e diff %.2e" % (extra, k, got[0][k], one[k], d))
    for k in KEYS:
        d = abs(got[0][k] - one[k])
        if extra == 0 and k in ("sdr", "sisdr", "l1_time", "separation_db", "input_sdr"):
            assert got[0][k] == one[k], (k, got[0][k], one[k])
        elif k in DB_KEYS:
            assert d < 1e-5, (k, got[0][k], one[k])
        else:
            assert d <= 1e-9 * abs(one[k]), (k, got[0][k], one[k])


@pytest.mark.parametrize("fill", [float("nan"), 1e30])
def test_nothing_behind_a_clips_end_is_read(model, batch, clean, fill):
    mix, speech, _ = batch
    dm, ds = np.array(mix), np.array(speech)
    for r0, ch, n in zip(FIRST, ROWS, LENS):
        dm[r0:r0 + ch, n:] = fill
        ds[r0:r0 + ch, n:] = fill
    got = model.evaluate_ragged(dev(dm), dev(ds), LENS, ROWS, return_estimate=True)
    a, b = np.array(numbers(got)), np.array(numbers(clean))
    print("tails filled with %r: largest |difference| of the 40 numbers %.3e" % (fill, np.abs(a - b).max()))
    assert a.shape == (5, 8) and np.isfinite(a).all()
    assert (a == b).all(), (a - b)
    for c in range(5):
        assert torch.equal(got[c]["x_time"], clean[c]["x_time"]), c


def test_run_equals_rerun_and_clip_order_does_not_matter(model, batch, clean):
    mix, speech, refs = batch
    again = model.evaluate_ragged(dev(mix), dev(speech), LENS, ROWS)
    assert numbers(again) == numbers(clean)                          # bit for bit: the same call shape, a fixed order of additions
    assert all("x_time" not in d for d in again)
    # the clips in reversed order (the longest last): every clip still within the bounds against its oracle
    order = [4, 3, 2, 1, 0]
    rm = np.concatenate([mix[FIRST[c]:FIRST[c] + ROWS[c]] for c in order])
    rs = np.concatenate([speech[FIRST[c]:FIRST[c] + ROWS[c]] for c in order])
    rev = model.evaluate_ragged(dev(rm), dev(rs), [LENS[c] for c in order], [ROWS[c] for c in order], return_estimate=True)
    for got, c in zip(rev, order):
        e = float((got["x_time"].cpu() - refs[c]["x_time"]).abs().max())
        print("reversed, clip %d: max|est - oracle| %.3e" % (c, e))
        assert e < EST_TOL
        compare(got, refs[c], "reversed, clip %d vs oracle:" % c)


def test_a_dirty_workspace_changes_nothing(sd_default, batch):
    mix, speech, _ = batch
    fresh = make_model(sd_default)
    expect = fresh.evaluate_ragged(dev(mix), dev(speech), LENS, ROWS, return_estimate=True)
    m = make_model(sd_default)
    nan_out = m.separate(torch.full((12, STRIDE + 2048), float("nan"), device="cuda"))     # NaN in, NaN out - and NaN all over a larger workspace
    assert torch.isnan(nan_out).all()
    got = m.evaluate_ragged(dev(mix), dev(speech), LENS, ROWS, return_estimate=True)
    a, b = np.array(numbers(got)), np.array(numbers(expect))
    print("after a NaN call: largest |difference| of the 40 numbers to a fresh context %.3e" % np.abs(a - b).max())
    assert np.isfinite(a).all() and (a == b).all(), (a - b)
    for c in range(5):
        assert torch.equal(got[c]["x_time"], expect[c]["x_time"]), c


def test_evaluate_many(model, batch):
    """The five pairs and a mono pair (clip 1's signals as 1-D tensors), some on the CPU; max_rows = 4 makes several buckets."""
    from speechseparation_amd import _native, metrics, spec
    mix, speech, refs = batch
    pairs, expect = [], []
    for c, (r0, ch, n) in enumerate(zip(FIRST, ROWS, LENS)):
        p = (torch.from_numpy(mix[r0:r0 + ch, :n].copy()), torch.from_numpy(speech[r0:r0 + ch, :n + (5 if c == 3 else 0)].copy()))
        pairs.append(p if c in (1, 3) else tuple(t.cuda() for t in p))         # (pair 3's clean signal is longer: cut to the common length)
        expect.append(refs[c])
    pairs.append((torch.from_numpy(mix[2, :LENS[1]].copy()).cuda(), torch.from_numpy(speech[2, :LENS[1]].copy())))
    expect.append(refs[1])
    buckets = spec.ragged_buckets([1 + n // 1024 for n in LENS + [LENS[1]]], ROWS + [1], 4, 0.25)
    assert len(buckets) >= 3
    outs = metrics.evaluate_many(model, pairs, max_rows=4)
    assert len(outs) == 6
    for i, (got, ref) in enumerate(zip(outs, expect)):
        assert set(got) == set(KEYS)
        compare(got, ref, "evaluate_many pair %d vs oracle:" % i)
    allocs = _native.lib.bsrnn_debug_counter(0)
    again = model.evaluate_many(pairs, max_rows=4)
    assert _native.lib.bsrnn_debug_counter(0) == allocs              # the same shapes again: no first-use work
    assert numbers(again) == numbers(outs)


def test_high_sdr_regime(sd_hot):
    """Targets close to the model's own output (SDR ~ 40 dB, where the noise sums are small differences): two clips of 12 and 5 frames.
    Bounds of tests/test_gpu_metrics.py::test_high_sdr_regime_and_reference_call_shape: 5e-3 dB, 5e-5 on the loss."""
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
    got = model.evaluate_ragged(dev(mix), dev(speech), lens, rows)
    for c, (g, ref) in enumerate(zip(got, refs)):
        assert ref["sdr"] > 20, ref["sdr"]
        compare(g, ref, "high SDR, clip %d vs oracle:" % c, db_tol=5e-3, rel_tol=5e-5)


def test_overlap_is_refused_and_a_clip_out_of_range_is_run_again(model, batch):
    """est_out over an input: BSRNN_EARG.  Then clip 3's mixture scaled by 3e7 drives its spectra beyond the fp16x2 operand range: the call
    returns rc 0 with every number finite, the other clips - run again in exact fp32 with it - within the bounds against the oracle.  For
    the scaled clip itself no bound can be derived here (its estimate is ~1e7 times its target): its differences to `evaluate` of that clip
    alone are printed, and only finiteness is asserted."""
    from speechseparation_amd import _native
    lib = _native.lib
    mix, speech, refs = batch
    wm, ws = dev(mix), dev(speech)
    ctx = model._context(torch.device("cuda", torch.cuda.current_device()))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    vals = (ctypes.c_double * 40)()
    cl, cr = (ctypes.c_int64 * 5)(*LENS), (ctypes.c_int32 * 5)(*ROWS)
    assert lib.bsrnn_evaluate_ragged(ctx, p(wm), p(ws), STRIDE, cl, cr, 5, p(wm), vals, None) == EARG
    assert b"overlap" in lib.bsrnn_last_error()
    assert lib.bsrnn_evaluate_ragged(ctx, p(wm), p(ws), STRIDE, cl, cr, 5, p(ws), vals, None) == EARG
    assert b"overlap" in lib.bsrnn_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(wm.cpu().numpy(), mix) and np.array_equal(ws.cpu().numpy(), speech)

    big = np.array(mix, np.float64)
    big[FIRST[3]:FIRST[3] + ROWS[3]] *= 3e7
    big = big.astype(np.float32)
    got = model.evaluate_ragged(dev(big), ws, LENS, ROWS, return_estimate=True)          # (a non-zero rc raises NativeError)
    a = np.array(numbers(got))
    assert np.isfinite(a).all(), a
    for c in (0, 1, 2, 4):
        e = float((got[c]["x_time"].cpu() - refs[c]["x_time"]).abs().max())
        print("clip %d beside the scaled one: max|est - oracle| %.3e" % (c, e))
        assert e < EST_TOL
        compare(got[c], refs[c], "clip %d beside the scaled one vs oracle:" % c)
    r0, ch, n = FIRST[3], ROWS[3], LENS[3]
    one = model.evaluate(dev(big[r0:r0 + ch, :n]), dev(speech[r0:r0 + ch, :n]), return_estimate=True)
    assert torch.isfinite(got[3]["x_time"]).all()
    print("scaled clip: max|ragged est - evaluate est| %.3e at |est|max %.3e" % (
        float((got[3]["x_time"] - one["x_time"]).abs().max()), float(one["x_time"].abs().max())))
    for k in KEYS:
        print("scaled clip %-13s ragged %.9e evaluate alone %.9e diff %.3e" % (k, got[3][k], one[k], abs(got[3][k] - one[k])))
    # nothing is left pending: the next call on the context succeeds
    model.evaluate_ragged(wm, ws, LENS, ROWS)


def test_validate_batch_rows(tmp_path):
    """validate.py --batch-rows 8 on three stereo file pairs of different lengths prints the two lines of the default invocation."""
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
    default, batched = run([]), run(["--batch-rows", "8"])
    for k in ("loss", "sdr", "input_sdr", "sisdr"):
        print("validate.py %-9s default %.8f --batch-rows 8 %.8f" % (k, default[k], batched[k]))
    assert abs(batched["loss"] - default["loss"]) <= REL_TOL * abs(default["loss"])
    for k in ("sdr", "input_sdr", "sisdr"):
        assert abs(batched[k] - default[k]) < DB_TOL, (k, batched[k], default[k])
