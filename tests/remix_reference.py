"""The definition of bsrnn_remix_ragged (include/bsrnn_hip.h) restated in numpy, float32 operation by float32 operation, for the tests:
a row is (n, [(src, at, gain), ...]) with src a 1-D float32 array (or None for a term of no samples), the first term the target."""
import numpy as np


def term_value(src, at, gain, n):
    """v_t(i) for i in [0, n): src[i - at] * gain inside the source, +0 outside; the product one float32 multiply."""
    v = np.zeros(n, np.float32)
    length = 0 if src is None else src.shape[0]
    lo, hi = max(0, at), min(n, at + length)
    if hi > lo:
        v[lo:hi] = src[lo - at:hi - at] * np.float32(gain)
    return v


def remix_rows(rows, width):
    """(mix, target) [R, width] float32: target = v_0, mix = v_0 + ((((+0 + v_1) + v_2) + ...), zeros from n to width."""
    mix = np.zeros((len(rows), width), np.float32)
    target = np.zeros((len(rows), width), np.float32)
    for r, (n, terms) in enumerate(rows):
        vals = [term_value(src, at, gain, n) for src, at, gain in terms]
        acc = np.zeros(n, np.float32)
        for v in vals[1:]:
            acc = acc + v
        target[r, :n] = vals[0]
        mix[r, :n] = vals[0] + acc
    return mix, target


def reads_of(rows):
    """Source samples the rows read, counted one by one (the traffic model's 4 bytes each)."""
    total = 0
    for n, terms in rows:
        for length, at in terms:
            total += sum(1 for i in range(n) if 0 <= i - at < length)
    return total


def reference_draws(idx, dialog_lengths, background_lengths, length, n_backgrounds=4):
    """MixDataSet.__getitem__'s draw sequence (m_dataset.py:149-176) written out on the GLOBAL generator, as the reference runs it, over
    sources that are lengths only: (dialog, backgrounds, offsets with the dialog first, gains of the backgrounds, the dialog's scale)."""
    import random
    dialogs = list(range(len(dialog_lengths)))
    backgrounds = list(range(len(background_lengths)))

    def random_resize(n):                       # m_dataset.py:129-139: where sample 0 of the source lands
        if n < length:
            return random.randint(0, length - n)
        return -random.randint(0, (n - length) - 1)

    random.seed(idx)
    random.choice(backgrounds)
    random.choice(backgrounds)
    dialog = random.choice(dialogs)
    random.choice(dialogs)
    random.choice(dialogs)
    random.choice(dialogs)
    chosen = [random.choice(backgrounds) for _ in range(n_backgrounds)]
    at = [random_resize(background_lengths[b]) for b in chosen]
    gains = [random.uniform(0.1, 1.0) for _ in chosen]
    scale = random.uniform(0.1, 1.0)
    at.insert(0, random_resize(dialog_lengths[dialog]))
    return dialog, chosen, at, gains, scale
