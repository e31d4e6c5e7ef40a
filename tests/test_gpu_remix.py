"""GPU: the re-mix of an optimizer step in one launch (bsrnn_remix_ragged; augment.SourceShelf / remix_draw / remix_many;
train.train_step_packed).  The definition fixes every rounding, so every comparison is bit for bit - torch.equal / array_equal on the bits -
against the numpy restatement of tests/remix_reference.py or against augment.remix, the torch code the call replaces.  Every call here
also holds the write bounds: a sentinel in front of the outputs, behind `width` in every row and behind the last row stays untouched."""
import ctypes
import random

import numpy as np
import pytest
import torch

import remix_reference as rr

pytestmark = pytest.mark.gpu

TILE = 2048
SENTINEL = 12345.0
DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what=""):
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), what


def _place(a, off):
    """The 1-D float32 array on the device, its base 16-byte aligned (off = 0) or `off` floats past such an address."""
    buf = torch.zeros(a.shape[0] + 8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + a.shape[0]]
    view.copy_(torch.from_numpy(a))
    return view


def run(rows, width, off=0, extra=None, src_off=0):
    """One bsrnn_remix_ragged: rows = [(n, [(src numpy array or None, at, gain), ...])].  The outputs start `off` floats past a 16-byte
    boundary with rows width + extra apart (extra None: up to the next multiple of 4); every source starts src_off floats past one.
    Returns (mix, target) [R, width] as numpy after checking every float around them."""
    from speechseparation_amd import _native, train
    dev = torch.device(DEV)
    R = len(rows)
    stride = width + ((-width) % 4 if extra is None else extra)
    keep, c_rows, c_terms = [], [], []
    for n, terms in rows:
        c_rows.append((n, len(c_terms), len(terms)))
        for src, at, gain in terms:
            if src is None or src.shape[0] == 0:
                c_terms.append((None, 0, at, gain, 0))
            else:
                t = _place(src, src_off)
                keep.append(t)
                c_terms.append((t.data_ptr(), src.shape[0], at, gain, 0))
    outs = []
    for _ in range(2):
        flat = torch.full((off + R * stride + 8,), SENTINEL, device=dev)
        assert flat.data_ptr() % 16 == 0
        outs.append(flat)
    mix, target = (f[off:off + R * stride].view(R, stride)[:, :width] for f in outs)
    _native.check(_native.lib.bsrnn_remix_ragged(train._context(dev), (_native.RemixRowC * R)(*c_rows), R, (_native.RemixTermC * len(c_terms))(*c_terms),
                                                 len(c_terms), train._p(mix), stride, train._p(target), stride, width, train._s(dev)))
    torch.cuda.synchronize()
    res = []
    for flat in outs:
        h = flat.cpu().numpy()
        body = h[off:off + R * stride].reshape(R, stride)
        assert (h[:off] == SENTINEL).all() and (h[off + R * stride:] == SENTINEL).all(), "written outside the rows"
        assert (body[:, width:] == SENTINEL).all(), "written behind width"
        res.append(body[:, :width].copy())
    for (n, _), m, t in zip(rows, res[0], res[1]):
        assert not _bits(m[n:]).any() and not _bits(t[n:]).any(), "columns [n, width) are +0"
    return res[0], res[1]


def check(rows, width, **kw):
    mix, target = run(rows, width, **kw)
    want_mix, want_target = rr.remix_rows(rows, width)
    _same_bits(target, want_target, "target")
    _same_bits(mix, want_mix, "mix")
    return mix, target


def _noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _gains(k, seed):
    r = random.Random(seed)
    return [r.uniform(0.1, 1.0) for _ in range(k)]


# ------------------------------------------------------------------------------------------------ shapes
def test_smallest_call():
    mix, target = check([(1, [(np.array([-1.5], np.float32), 0, 1.0)])], 1)
    assert mix[0, 0] == -1.5 and target[0, 0] == -1.5


def test_row_lengths_around_the_tile():
    lens = [1, 255, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 5]
    width = 3 * TILE + 5
    rows = []
    for r, n in enumerate(lens):
        g = _gains(2, r)
        rows.append((n, [(_noise(n + 9, 10 + r), -4, 1.0),                        # a dialog cut on both sides
                         (_noise(max(1, n // 2), 20 + r), n // 3, g[0]),           # padded on both sides
                         (_noise(n + 700, 30 + r), -(r + 1), g[1])]))              # cut, at = -1 ... -7
    check(rows, width)
    for n in lens:                                                                 # and each as a call of its own width
        check([(n, [(_noise(n, 40), 0, 1.0), (_noise(n + 3, 41), -3, 0.7)])], n)


def test_placements_and_offsets_mod_4():
    n = 2 * TILE + 77
    rows = []
    for a in range(4):                                                             # at = a, a + 4 k: every residue, padding and cuts
        short, long_ = _noise(TILE + 13, 50 + a), _noise(n + 1000 + a, 60 + a)
        g = _gains(6, a)
        rows.append((n, [(_noise(n, 70 + a), 0, 1.0),
                         (short, n - short.shape[0], g[0]),                        # padding on the left only
                         (short, 0, g[1]),                                         # on the right only
                         (short, 4 * 100 + a, g[2]),                               # on both sides
                         (long_, 0, g[3]),                                         # cut at 0
                         (long_, -(long_.shape[0] - n), g[4]),                     # cut at the very end
                         (long_, -(4 * 50 + a), g[5])]))                           # somewhere inside
    rows.append((n, [(_noise(50, 80), -50, 1.0), (_noise(50, 81), n, 0.5), (_noise(50, 82), -49, 0.5), (_noise(50, 83), n - 1, 0.5)]))   # just outside, one sample inside
    check(rows, n + 10)


def test_aligned_and_misaligned_calls_give_the_same_bits():
    n = TILE + 301
    rows = [(n, [(_noise(n + 40, 90), -8, 1.0), (_noise(900, 91), 16, 0.37), (_noise(n + 64, 92), -12, 0.81)]),
            (n - 5, [(_noise(n, 93), 0, 1.0), (_noise(n, 94), -4, 0.22)])]
    a = check(rows, n, off=0, extra=(-n) % 4, src_off=0)           # every source and both outputs on 16-byte boundaries, strides a multiple of 4
    b = check(rows, n, off=1, extra=3, src_off=1)                  # everything one float off, rows width + 3 apart
    _same_bits(a[0], b[0])
    _same_bits(a[1], b[1])


def test_write_bounds_and_zero_columns():
    n = TILE + 9
    rows = [(n, [(_noise(n, 100), 0, 1.0), (_noise(n, 101), 0, 0.5)]), (0, [(_noise(40, 102), 0, 1.0)]), (1, [(_noise(40, 103), 0, 1.0)]),
            (TILE, [(None, 0, 1.0), (_noise(TILE + 50, 104), -50, 0.9)])]
    for off, extra in ((0, 0), (3, 5), (2, 1)):
        mix, target = check(rows, n + 700, off=off, extra=extra)   # (run() holds the sentinels and the zeros behind n)
    assert not _bits(mix[1]).any() and not _bits(target[1]).any() and not _bits(target[3]).any()


# ------------------------------------------------------------------------------------------------ rounding
def test_rounding_order_is_python_sum():
    """dialog + sum(backgrounds) with four scaled backgrounds, against torch on the CPU doing literally that.  A multiply fused into the
    addition, or another summation order, changes about a fifth of the samples: both are shown to differ here, so the test can tell."""
    n = 4099
    d = _noise(n, 110)
    bg = [_noise(n, 111 + k) for k in range(4)]
    g = _gains(4, 5)
    want = torch.from_numpy(d) + sum([torch.from_numpy(x) * s for x, s in zip(bg, g)])
    mix, target = check([(n, [(d, 0, 1.0)] + [(x, 0, s) for x, s in zip(bg, g)])], n)
    assert torch.equal(torch.from_numpy(mix[0]), want) and np.array_equal(_bits(target[0]), _bits(d))
    g32 = [np.float32(s) for s in g]
    fused = np.zeros(n, np.float32)
    for x, s in zip(bg, g32):
        fused = (x.astype(np.float64) * np.float64(s) + fused.astype(np.float64)).astype(np.float32)      # one rounding per term
    fused = d + fused
    assert 0.05 < float((_bits(fused) != _bits(mix[0])).mean()) < 0.6
    backwards = d + (((bg[3] * g32[3] + bg[2] * g32[2]) + bg[1] * g32[1]) + bg[0] * g32[0])
    assert 0.05 < float((_bits(backwards) != _bits(mix[0])).mean()) < 0.6


def test_signed_zero():
    neg = np.array([-0.0, 0.0, -0.0, 1.0], np.float32)
    mix, target = check([(4, [(neg, 0, 1.0)])], 6)
    assert list(np.signbit(target[0])) == [True, False, True, False, False, False]
    assert not np.signbit(mix[0]).any()
    mix, target = check([(4, [(neg, 0, 1.0), (neg, 0, 0.5)])], 4)              # -0 + (0 + -0) = +0 as well
    assert not np.signbit(mix[0]).any() and list(np.signbit(target[0])) == [True, False, True, False]


def test_special_values_pass_through_by_position():
    n = 300
    d, b = _noise(n, 120), _noise(n, 121)
    d[7], d[100], b[100], b[200], b[299] = np.inf, np.nan, 1.0, -np.inf, np.nan
    mix, target = run([(n, [(d, 0, 1.0), (b, 0, 0.5)])], n)
    want_mix, want_target = rr.remix_rows([(n, [(d, 0, 1.0), (b, 0, 0.5)])], n)
    assert np.array_equal(np.isnan(mix[0]), np.isnan(want_mix[0])) and list(np.flatnonzero(np.isnan(mix[0]))) == [100, 299]
    assert np.array_equal(np.isnan(target[0]), np.isnan(d)) and target[0, 7] == np.inf and mix[0, 7] == np.inf and mix[0, 200] == -np.inf
    ok = ~np.isnan(want_mix[0])
    assert np.array_equal(_bits(mix[0][ok]), _bits(want_mix[0][ok])) and np.array_equal(_bits(target[0][~np.isnan(d)]), _bits(d[~np.isnan(d)]))


def test_rows_in_a_batch_equal_rows_alone():
    counts = [1, 2, 5, 9, 3]
    n = TILE + 123
    rows = []
    for r, c in enumerate(counts):
        g = _gains(c, 130 + r)
        terms = [(_noise(n + 17 * k, 140 + 10 * r + k), -(5 * k + r), 1.0 if k == 0 else g[k]) for k in range(c)]
        rows.append((n - 11 * r, terms))
    mix, target = check(rows, n)
    for r, row in enumerate(rows):
        m1, t1 = run([row], n)
        _same_bits(m1[0], mix[r], r)
        _same_bits(t1[0], target[r], r)


# ------------------------------------------------------------------------------------------------ the Python layer
def _stereo(n, seed):
    return torch.from_numpy(np.stack([_noise(n, seed), _noise(n, seed + 1000)]))


def test_mono_source_feeds_both_rows_through_one_pointer():
    from speechseparation_amd import augment
    shelf = augment.SourceShelf(DEV)
    mono = torch.from_numpy(_noise(3000, 150))
    shelf.add_dialog(mono)                                       # [n]: mono
    shelf.add_background(_stereo(7000, 151))
    shelf.add_background(torch.from_numpy(_noise(2000, 152))[None])          # [1, n]: mono as well
    assert (len(shelf), shelf.n_dialogs, shelf.n_backgrounds) == (3, 1, 2)
    assert shelf.length_of("dialog", 0) == 3000 and shelf.length_of("background", 1) == 2000 and shelf.channels_of("background", 0) == 2
    spec = augment.RemixSpec(0, (0, 1), (100, -500, 1700), (1.0, 0.4, 0.9), 4000)
    mix, target, lengths, clip_rows = augment.remix_many(shelf, [spec], 4000)
    assert lengths == [4000] and clip_rows == [2] and tuple(mix.shape) == tuple(target.shape) == (2, 4000)
    assert torch.equal(target[0], target[1]) and not torch.equal(mix[0], mix[1])
    d = shelf._rows("dialog", 0)[0].cpu().numpy()
    b0, b1 = (shelf._rows("background", 0)[c].cpu().numpy() for c in range(2))
    m = shelf._rows("background", 1)[0].cpu().numpy()
    want_mix, want_target = rr.remix_rows([(4000, [(d, 100, 1.0), (b0, -500, 0.4), (m, 1700, 0.9)]),
                                           (4000, [(d, 100, 1.0), (b1, -500, 0.4), (m, 1700, 0.9)])], 4000)
    _same_bits(mix.cpu().numpy(), want_mix)
    _same_bits(target.cpu().numpy(), want_target)
    # a given pair of outputs goes by pointer, with its row stride
    flat = [torch.full((2 * 4003 + 1,), SENTINEL, device=DEV) for _ in range(2)]
    out = tuple(f[1:].view(2, 4003)[:, :4000] for f in flat)
    got = augment.remix_many(shelf, [spec], 4000, out=out)
    assert got[0].data_ptr() == out[0].data_ptr() and torch.equal(out[0], mix) and torch.equal(out[1], target)
    for f in flat:
        assert float(f[0]) == SENTINEL and bool((f[1:].view(2, 4003)[:, 4000:] == SENTINEL).all())
    with pytest.raises(ValueError):
        augment.remix_many(shelf, [spec], 4001)


def test_end_to_end_against_augment_remix_and_one_training_loss(sd_default):
    from speechseparation_amd import augment, train
    from speechseparation_amd.bsrnn import BSRNN
    length = 5000
    dialogs = [_stereo(3000, 160), torch.from_numpy(_noise(9000, 161))[None], _stereo(6500, 162)]
    backgrounds = [_stereo(4200, 163), torch.from_numpy(_noise(7700, 164))[None], _stereo(8999, 165)]
    shelf = augment.SourceShelf(DEV)
    for t in dialogs:
        shelf.add_dialog(t)                                      # CPU tensors: uploaded once
    for t in backgrounds:
        shelf.add_background(t.to(DEV))                          # device tensors: kept by reference
    assert shelf._rows("background", 0)[0].device.type == "cuda" and len(shelf) == 6
    two = lambda t: torch.cat((t, t), 0) if t.shape[0] == 1 else t          # noqa: E731  m_dataset.load_waveform
    indices = [0, 1, 2]
    specs = [augment.remix_draw(idx, shelf, length) for idx in indices]
    mix, target, lengths, clip_rows = augment.remix_many(shelf, specs, length)
    assert lengths == [length] * 3 and clip_rows == [2, 2, 2] and tuple(mix.shape) == (6, length)
    for c, idx in enumerate(indices):
        rng = random.Random(idx)
        rng.choice(range(3)), rng.choice(range(3))                           # the two unused backgrounds
        dialog = rng.choice(range(3))
        rng.choice(range(3)), rng.choice(range(3)), rng.choice(range(3))     # three unused dialogs
        chosen = [rng.choice(range(3)) for _ in range(4)]
        assert (dialog, chosen) == (specs[c].dialog, list(specs[c].backgrounds))
        want_mix, want_target = augment.remix(two(dialogs[dialog]).to(DEV), [two(backgrounds[b]).to(DEV) for b in chosen], length, rng)
        assert torch.equal(mix[2 * c:2 * c + 2], want_mix) and torch.equal(target[2 * c:2 * c + 2], want_target), idx
    model = BSRNN().train()
    model.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd_default.items()})
    model = model.to(DEV)
    losses, sdrs, _ = train.train_loss_ragged(model, mix, target, lengths, clip_rows)
    assert tuple(losses.shape) == (3,) and bool(torch.isfinite(losses).all()) and bool(torch.isfinite(sdrs).all())
    opt = train.AdamW(model.parameters())
    before = [p.detach().clone() for p in model.parameters() if p.numel() > 0]
    vals = train.train_step_packed(model, opt, mix, target, lengths, clip_rows)
    assert len(vals) == 3 and all(np.isfinite(v[0]) and np.isfinite(v[1]) for v in vals)
    assert [v[0] for v in vals] == pytest.approx(losses.detach().cpu().tolist(), rel=1e-4)       # the same losses, before the step
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, (p for p in model.parameters() if p.numel() > 0)))
    assert all(p.grad is None for p in model.parameters())


def test_train_py_remix_runs_an_epoch(tmp_path, capsys):
    """train.py --remix on a folder of small WAV files, in this process: listing, shelf, draws, one launch per step, the packed step."""
    import importlib.util
    import os
    from conftest import REPO
    from speechseparation_amd import audio
    spec_ = importlib.util.spec_from_file_location("train_entry_remix_gpu", os.path.join(REPO, "train.py"))
    entry = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(entry)
    data, out = tmp_path / "data", tmp_path / "out"
    (data / "film").mkdir(parents=True)
    out.mkdir()
    files = {"speech.wav": _stereo(3000, 180), "film/dialog-2048.wav": torch.from_numpy(_noise(7000, 181))[None],
             "film/dialog-9216.wav": torch.from_numpy(_noise(2500, 182))[None], "sfx.wav": _stereo(9000, 183),
             "film/background-4096.wav": torch.from_numpy(_noise(1500, 184))[None], "music.wav": _stereo(5200, 185)}
    for name, w in files.items():
        audio.save_wav(str(data / name), 0.1 * w, 44100)
    entry.main(["--remix", str(data), "--remix_seconds", "0.1", "--remix_backgrounds", "3", "--batch_size", "2", "--synthetic-weights", "0",
                "--outdir", str(out), "--device", DEV])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("Epoch 0 Loss")]
    assert len(line) == 1, text
    loss, sdr = float(line[0].split()[3]), float(line[0].split()[5])
    assert np.isfinite(loss) and np.isfinite(sdr) and loss > 0
    assert os.path.exists(out / "model-always.pth") and os.path.exists(out / "optimizer-always.pth")


def test_section_views_give_the_bits_of_copies():
    from speechseparation_amd import augment, mining
    wave = torch.from_numpy(_noise(14 * 1024 + 100, 170)).to(DEV)
    sections = [mining.Section(mining.DIALOG, 0, 3), mining.Section(mining.BACKGROUND, 4, 9), mining.Section(mining.DIALOG, 9, 11),
                mining.Section(mining.BACKGROUND, 11, 14)]
    views, copies = augment.SourceShelf(DEV), augment.SourceShelf(DEV)
    assert views.add_sections(wave, sections) == (2, 2)
    assert views.add_sections(wave, mining.Mined([sections[:2]], np.zeros((1, 14, 2)))) == (1, 1)      # what mining.mine returns for a clip
    for s in sections + sections[:2]:
        a, b = s.samples
        (copies.add_dialog if s.kind == mining.DIALOG else copies.add_background)(wave[a:b].clone())
    assert views._rows("dialog", 1)[0].data_ptr() == wave.data_ptr() + 4 * 9 * 1024          # a view: no copy
    assert views.length_of("background", 0) == 5 * 1024 and (views.n_dialogs, views.n_backgrounds) == (3, 3)
    length = 4000
    specs = [augment.remix_draw(idx, views, length, n_backgrounds=2) for idx in range(3)]
    a = augment.remix_many(views, specs, length)
    b = augment.remix_many(copies, specs, length)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:] == b[2:] and bool(a[0].abs().sum() > 0)
    with pytest.raises(ValueError):
        views.add_sections(wave, [mining.Section(mining.DIALOG, 10, 15)])       # ends behind the recording
