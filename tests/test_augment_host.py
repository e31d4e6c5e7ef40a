"""CPU-side tests of the training augmentations' host parts (speechseparation_amd/augment.py): rir_draw against the reference's sequence of
draws on the global generator (m_dataset.py:83-102), remix against MixDataSet's arithmetic (:123-178) bit for bit, and train.py's new
flags.  The convolution itself: tests/test_gpu_convolve.py, tests/test_gpu_augment.py."""
import random

import torch

RIRS = ["room%02d_imp.wav" % i for i in range(7)]
CHANNELS = [1, 2, 8, 4, 2, 1, 6]


def reference_draw(idx):
    """What MyDataSet.__getitem__ decides for clip idx, on the global generator as it does (the response's channel count stands in for the
    file it reads)."""
    random.seed(idx)
    if not random.choices([True, False], weights=[0.1, 0.9])[0]:
        return None
    name = random.choices(RIRS)[0]
    n_ch = CHANNELS[RIRS.index(name)]
    first = random.randint(0, n_ch - 1)
    second = random.randint(0, n_ch - 1)
    return RIRS.index(name), first, second


def test_rir_draw_is_the_reference_sequence():
    from speechseparation_amd.augment import rir_draw
    want = [reference_draw(idx) for idx in range(200)]
    state = random.getstate()
    got = [rir_draw(idx, len(RIRS), CHANNELS.__getitem__) for idx in range(200)]
    assert random.getstate() == state                       # its own generator: the caller's global one is not touched
    assert got == want
    hits = sum(d is not None for d in want)
    print("reference draws True for %d of 200 indices" % hits)
    assert 5 <= hits <= 40                                   # some do, most do not (p = 0.1)
    assert len({d[0] for d in want if d}) > 1 and any(d[1] != d[2] for d in want if d)
    # the probability is the caller's
    assert all(rir_draw(idx, 7, CHANNELS.__getitem__, prob=1.0) is not None for idx in range(50))
    assert all(rir_draw(idx, 7, CHANNELS.__getitem__, prob=0.0) is None for idx in range(50))


def reference_resize(x, length):
    """m_dataset.random_resize on the global generator: zero columns on both sides, split at random, or a random cut."""
    if x.shape[1] < length:
        missing = length - x.shape[1]
        left = random.randint(0, missing)
        col = torch.zeros((x.shape[0], 1))
        return torch.cat((col.repeat((1, left)), x, col.repeat((1, missing - left))), dim=1)
    left = random.randint(0, x.shape[1] - length - 1)
    return x[:, left:left + length]


def reference_mix(dialog, backgrounds, length):
    """MixDataSet.__getitem__ from the loaded tensors on (m_dataset.py:163-178)."""
    backgrounds = [reference_resize(b, length) for b in backgrounds]
    backgrounds = [b * random.uniform(0.1, 1.0) for b in backgrounds]
    random.uniform(0.1, 1.0)                                 # the dialog's scale: drawn, its use is commented out
    dialog = reference_resize(dialog, length)
    return dialog + sum(backgrounds), dialog


def test_remix_is_the_reference_arithmetic():
    from speechseparation_amd.augment import remix
    g = torch.Generator().manual_seed(3)
    length = 5000
    for seed, sizes, n_dialog in ((0, (3000, 7000, 5001, 4999), 6000), (1, (9000, 100, 5002, 20000), 1200), (2, (1, 12000), 4999)):
        backgrounds = [torch.randn((2, n), generator=g) for n in sizes]
        dialog = torch.randn((2, n_dialog), generator=g)
        random.seed(seed)
        want_mix, want_dialog = reference_mix(dialog, backgrounds, length)
        after = random.random()
        rng = random.Random(seed)
        mix, dlg = remix(dialog, backgrounds, length, rng)
        assert rng.random() == after                         # the same number of draws, in the same order
        assert mix.shape == (2, length) and torch.equal(mix, want_mix) and torch.equal(dlg, want_dialog)
        random.seed(seed)                                    # the global module serves as rng too
        mix2, _ = remix(dialog, backgrounds, length, random)
        assert torch.equal(mix2, want_mix)


def test_train_flags():
    import train
    ap = train.build_parser()
    args = ap.parse_args(["--synthetic", "4"])
    assert args.rir is None and args.rir_prob == 0.1 and args.rir_rate == 16000
    args = ap.parse_args(["--synthetic", "4", "--rir", "/some/dir", "--rir_prob", "0.5", "--rir_rate", "48000", "--ragged", "--batch_size", "4"])
    assert (args.rir, args.rir_prob, args.rir_rate, args.ragged, args.batch_size) == ("/some/dir", 0.5, 48000, True, 4)
    doc = train.__doc__
    assert "--rir" in doc and "m_dataset.py:92-114" in doc and "RIR / re-mix augmentations" not in doc
