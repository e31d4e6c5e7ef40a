"""GPU: section mining on the device path (speechseparation_amd.mining, gendataset-separate.py) against tests/sections_reference.py.

(a) constructed signals that take every branch of the state machine: est = g[h] * mix per hop.  With a Gaussian mixture of sigma 0.1,
    10 ln mean(e^2 / (w - e)^2) is 43.94 for g = 0.9, 21.97 for 0.75, 4.01 for 0.55, 0.00 for 0.5 and -91.90 for 0.01 - none anywhere near a
    threshold (10, 3, -30); a hop of mix * 1e-5 has a level mean of about 1e-12, below the floor of 1e-10.  hop_activity -> SectionScanner
    must give exactly the sections the restatement gives from the numpy activity.
(b) `mine` on three clips of 12, 30 (two rows) and 41 hops with segments of 8 frames and synthetic weights: the returned activity against
    the restatement's activity of the mixture and of `separate_many_long`'s own result, at the activity test's tolerance (relative 1e-12:
    the same 1024 fp32 terms added in double in another order); the returned sections against the restatement's scan of that activity;
    input order; one hop_activity and one separation per bucket, counted through a wrapper around the library object.
(c) the script end to end on WAV files in tmp_path: file names and lengths follow first_hop / end_hop."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import sections_reference as sr
from conftest import REPO

pytestmark = pytest.mark.gpu
HOP = 1024
SILENT, SAME, ZERO = "silent", "same", "zero"
# (what, hops): g = est / mix of the hop; SILENT: mix * 1e-5 with g = 0.5; SAME: est == mix (+inf); ZERO: both zero (NaN, level 0)
PLAN = [(0.9, 12),                    # dialog opens at hop 9
        (0.55, 2), (SILENT, 2),       # bridged by db, then by silence
        (0.9, 1), (0.5, 1),           # dialog again, then neither: the section closes
        (0.01, 12),                   # background opens
        (SAME, 3),                    # +inf is dialog: closes the background section
        (0.5, 1),                     # reset
        (0.75, 11), (0.01, 12),       # dialog -> background directly
        (0.9, 5), (0.55, 1),          # a bridge hop with n_dialog < min_run resets
        (0.9, 5), (SILENT, 1),        # so does a silent one
        (0.01, 9), (ZERO, 3),         # nine background hops are no section; digital silence resets
        (0.9, 12)]                    # open at the end: closed by the flush


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


def constructed():
    n_hops = sum(n for _, n in PLAN)
    rng = np.random.RandomState(42)
    w = (0.1 * rng.randn(n_hops, HOP)).astype(np.float32)
    e = np.empty_like(w)
    h = 0
    for what, n in PLAN:
        for _ in range(n):
            if what == SILENT:
                w[h] *= np.float32(1e-5)
                e[h] = w[h] * np.float32(0.5)
            elif what == SAME:
                e[h] = w[h]
            elif what == ZERO:
                w[h] = 0.0
                e[h] = 0.0
            else:
                e[h] = w[h] * np.float32(what)
            h += 1
    return w.reshape(1, -1), e.reshape(1, -1)


def test_constructed_signals_take_every_branch(model):
    from speechseparation_amd import mining
    w, e = constructed()
    want_act = sr.activity(w, e)
    assert sr.clear_of_thresholds(want_act[0], margin=1e-6)
    # the figures of the table above, and the silent hops' level
    dbs = {what: sr.to_db(float(want_act[0, h, 0])) for what, h in ((0.9, 0), (0.55, 12), (0.5, 17), (0.01, 18), (0.75, 34))}
    for g, db in ((0.9, 43.94), (0.75, 21.97), (0.55, 4.01), (0.5, 0.0), (0.01, -91.90)):
        assert abs(dbs[g] - db) < 0.02, (g, dbs[g])
    assert want_act[0, 14, 1] < 1e-10 and np.isposinf(want_act[0, 30, 0]) and np.isnan(want_act[0, 78, 0])
    want = sr.scan(want_act[0])
    assert want == [(1, 9, 17), (2, 27, 30), (1, 43, 45), (2, 54, 57), (1, 90, 93)]
    act = mining.hop_activity(model, torch.from_numpy(w).cuda(), torch.from_numpy(e).cuda())
    sr.compare_activity(act.cpu().numpy(), want_act, "constructed signals")
    sc = mining.SectionScanner()
    got = sc.feed(act[0], flush=True)
    assert [tuple(s) for s in got] == want
    # and as a stream: a few hops per feed, the flush at the end
    sc.reset()
    got = [s for a in range(0, act.shape[1], 7) for s in sc.feed(act[0, a:a + 7])] + sc.flush()
    assert [tuple(s) for s in got] == want


class CountingLib:
    """The library object with a count of the calls made through it, by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


@pytest.fixture(scope="module")
def clips():
    from speechseparation_amd import weights
    return [torch.from_numpy(weights.synth_waveform(1, 12 * HOP + 7, seed=21)[0].copy()),
            torch.from_numpy(weights.synth_waveform(2, 30 * HOP, seed=22).copy()),
            torch.from_numpy(weights.synth_waveform(1, 41 * HOP + 1000, seed=23)[0].copy())]


def test_mine_three_clips(model, clips, monkeypatch):
    from speechseparation_amd import bsrnn, mining
    counting = CountingLib(mining._lib)
    monkeypatch.setattr(mining, "_lib", counting)
    monkeypatch.setattr(bsrnn, "_lib", counting)
    mined = mining.mine(model, clips, segment_frames=8)
    assert counting.calls.get("bsrnn_hop_activity") == 1 and counting.calls.get("bsrnn_separate_long_ragged") == 1      # one bucket
    monkeypatch.undo()
    est = model.separate_many_long(clips, segment_frames=8)
    assert len(mined) == 3
    for i, (clip, m, y) in enumerate(zip(clips, mined, est)):
        rows = clip.reshape(-1, clip.shape[-1]).numpy()
        H = rows.shape[1] // HOP
        assert m.activity.shape == (rows.shape[0], H, 2) and m.activity.dtype == np.float64 and len(m.sections) == rows.shape[0]      # input order
        want = sr.activity(rows[:, :H * HOP], y.reshape(rows.shape[0], -1).numpy())
        sr.compare_activity(m.activity, want, "clip %d" % i)
        for r in range(rows.shape[0]):
            dbs = [sr.to_db(float(v)) for v in want[r, :, 0]]
            print("clip %d row %d: db min %.2f max %.2f, sections %s" % (i, r, min(dbs), max(dbs), [tuple(s) for s in m.sections[r]]))
            assert sr.clear_of_thresholds(m.activity[r], margin=1e-6)
            assert [tuple(s) for s in m.sections[r]] == sr.scan(m.activity[r])


def test_mine_one_call_per_bucket(model, clips, monkeypatch):
    from speechseparation_amd import bsrnn, mining, spec
    buckets = spec.long_buckets([spec.n_frames(c.shape[-1]) for c in clips], [1, 2, 1], 2)
    assert buckets == [[2], [1], [0]]
    counting = CountingLib(mining._lib)
    monkeypatch.setattr(mining, "_lib", counting)
    monkeypatch.setattr(bsrnn, "_lib", counting)
    mined = mining.mine(model, clips, segment_frames=8, max_rows=2, rule=mining.SectionRule(min_run=2))
    assert counting.calls.get("bsrnn_hop_activity") == 3 and counting.calls.get("bsrnn_separate_long_ragged") == 3
    assert [m.activity.shape for m in mined] == [(1, 12, 2), (2, 30, 2), (1, 41, 2)]
    for m in mined:
        for r, sections in enumerate(m.sections):
            assert [tuple(s) for s in sections] == sr.scan(m.activity[r], min_run=2)


def test_script_end_to_end(model, tmp_path):
    """gendataset-separate.py on two WAV files (one at 22.05 kHz: resampled to 44.1 kHz): the files it writes are the mono mixture of the
    sections `mine` finds for the chosen channel, named by the reference's sample counter."""
    from speechseparation_amd import audio, mining, weights
    spec_ = importlib.util.spec_from_file_location("gendataset_separate", os.path.join(REPO, "gendataset-separate.py"))
    script = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(script)
    a = torch.from_numpy(weights.synth_waveform(2, 40 * HOP + 300, seed=31).copy())
    b = torch.from_numpy(weights.synth_waveform(1, 15 * HOP, seed=32).copy())
    audio.save_wav(str(tmp_path / "a.wav"), a, 44100)
    audio.save_wav(str(tmp_path / "b.wav"), b, 22050)
    out = tmp_path / "out"
    script.main(["--input", str(tmp_path / "a.wav"), "--input", str(tmp_path / "b.wav"), "--output", str(out), "--channel", "0",
                 "--synthetic-weights", "0", "--segment-frames", "8"])
    assert torch.is_grad_enabled(), "the script's main leaves the process as it found it"
    clips = [audio.load_wav(str(tmp_path / "a.wav"))[0][0], audio.resample(audio.load_wav(str(tmp_path / "b.wav"))[0][:1], 22050, 44100)[0]]
    assert clips[1].shape[0] == 30 * HOP
    mined = mining.mine(model, clips, segment_frames=8)
    n_files = 0
    for name, clip, m in zip(("a", "b"), clips, mined):
        want = {"%s-%d.wav" % (s.name, (s.first_hop + 1) * HOP): s for s in m.sections[0]}
        assert sorted(os.listdir(out / name)) == sorted(want)
        for fname, s in want.items():
            data, rate = audio.load_wav(str(out / name / fname))
            assert rate == 44100 and data.shape == (1, (s.end_hop - s.first_hop) * HOP)
            assert torch.equal(data[0], clip[s.first_hop * HOP:s.end_hop * HOP])
            n_files += 1
    print("script: %d section files" % n_files)
    # one input: the files lie in --output itself
    single = tmp_path / "single"
    script.main(["--input", str(tmp_path / "a.wav"), "--output", str(single), "--channel", "1", "--synthetic-weights", "0",
                 "--segment-frames", "8"])
    m = mining.mine(model, [audio.load_wav(str(tmp_path / "a.wav"))[0][1]], segment_frames=8)[0]
    assert sorted(os.listdir(single)) == sorted("%s-%d.wav" % (s.name, (s.first_hop + 1) * HOP) for s in m.sections[0])
