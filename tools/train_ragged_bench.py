#!/usr/bin/env python3
"""One optimizer step over B stereo clips, two ways, in one process on one GPU, inputs resident, after a warm-up of every shape:

  (a) clip by clip          the loop of train.py without --ragged: per clip train_loss, sdr, backward() and the two figures read back,
                            then AdamW.step() and zero_grad() - B passes of 2 rows
  (b) train_step_many       spec.ragged_buckets with the defaults (64 rows, padding share <= 0.25), per bucket one train_loss_ragged and
                            one backward(), the packing copies and the read-back included, then the same optimizer step

for B in {4, 16, 32}, once with equal clips of 8 s at 16 kHz and once with lengths spread evenly over 4 .. 8 s (shuffled).  Each figure is
the median of REPEATS steps on a host clock, min .. max beside it; (a) and (b) alternate inside every repeat.  Also printed: the padding
share of (b), torch.cuda.max_memory_allocated of each variant, bsrnn_debug_counter(0) around a second step of (b) that fits, and for the
largest case the stages of (b) on device events.

    python tools/train_ragged_bench.py [--out profiles/train_ragged_step.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (4, 16, 32)
RATE, CHANNELS = 16000, 2
REPEATS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speechseparation_amd import _native, spec, train, weights
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = weights.synth_state_dict(None, seed=0)

    def fresh():
        m = BSRNN().train()
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m = m.to("cuda:0")
        return m, train.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)

    def make_pairs(lens):
        out = []
        for i, n in enumerate(lens):
            speech = weights.synth_waveform(CHANNELS, n, seed=140 + i, scale=0.07)
            mix = speech + weights.synth_waveform(CHANNELS, n, seed=40 + i, scale=0.05)
            out.append((torch.from_numpy(mix).cuda(), torch.from_numpy(speech).cuda()))
        return out

    def step_a(model, opt, pairs):
        out = []
        for mix, speech in pairs:
            loss, x_time = train.train_loss(model, mix, speech)
            s = train.sdr(x_time, speech[:, :x_time.shape[1]])
            loss.backward()
            out.append((float(loss.detach()), float(s.detach())))
        opt.step()
        opt.zero_grad()
        return out

    def step_b(model, opt, pairs):
        return train.train_step_many(model, opt, pairs)

    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# ms per optimizer step over B clips x %d channels: median [min .. max] of %d steps; peak = torch.cuda.max_memory_allocated" % (CHANNELS, REPEATS))
    say("%-12s %4s %8s %8s %28s %28s %7s %9s %9s" % ("lengths", "B", "buckets", "padding", "(a) clip by clip, ms", "(b) train_step_many, ms", "a / b",
                                                   "peak a MB", "peak b MB"))
    largest = None
    for tag in ("equal 8 s", "4 .. 8 s"):
        for B in BATCHES:
            if tag == "equal 8 s":
                lens = [8 * RATE] * B
            else:
                lens = [int(round(4 * RATE + i * 4 * RATE / max(1, B - 1))) for i in range(B)]
                lens = [lens[i] for i in np.random.RandomState(3).permutation(B)]       # a training set does not arrive sorted
            pairs = make_pairs(lens)
            frames = [spec.n_frames(n) for n in lens]
            buckets = spec.ragged_buckets(frames, [CHANNELS] * B, 64, 0.25)
            padding = 1 - sum(frames) / sum(len(b) * max(frames[i] for i in b) for b in buckets)
            (ma, oa), (mb, ob) = fresh(), fresh()
            ra, rb = step_a(ma, oa, pairs), step_b(mb, ob, pairs)                       # warm-up of every shape; the same figures, to rounding
            e = max(abs(x[0] - y[0]) / abs(x[0]) for x, y in zip(ra, rb))
            assert e < 1e-5, e
            t, peak = {"a": [], "b": []}, {}
            for k, (f, m, o) in (("a", (step_a, ma, oa)), ("b", (step_b, mb, ob))):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                f(m, o, pairs)
                torch.cuda.synchronize()
                peak[k] = torch.cuda.max_memory_allocated() / 2 ** 20
            allocs = _native.lib.bsrnn_debug_counter(0)
            step_b(mb, ob, pairs)
            moved = _native.lib.bsrnn_debug_counter(0) - allocs
            for _ in range(REPEATS):
                for k, (f, m, o) in (("a", (step_a, ma, oa)), ("b", (step_b, mb, ob))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f(m, o, pairs)
                    torch.cuda.synchronize()
                    t[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: float(np.median(v)) for k, v in t.items()}
            say("%-12s %4d %8d %8.3f %10.2f [%6.2f .. %7.2f] %10.2f [%6.2f .. %7.2f] %7.2f %9.0f %9.0f" % (
                tag, B, len(buckets), padding, med["a"], min(t["a"]), max(t["a"]), med["b"], min(t["b"]), max(t["b"]), med["a"] / med["b"],
                peak["a"], peak["b"]))
            say("#   bsrnn_debug_counter(0) moved by %d during a second step of (b)" % moved)
            if tag == "equal 8 s" and B == BATCHES[-1]:
                largest = (mb, pairs, lens)

    # the stages of (b) for the largest equal-length case, on device events (one bucket: 64 rows x 126 frames)
    model, pairs, lens = largest
    mix, speech = torch.stack([p[0] for p in pairs]).reshape(-1, lens[0]), torch.stack([p[1] for p in pairs]).reshape(-1, lens[0])
    rows = [CHANNELS] * len(pairs)
    row_lens = [n for n in lens for _ in range(CHANNELS)]
    marks = []

    def mark(name):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append((name, ev))
    for rep in range(3):
        marks.clear()
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        mark("start")
        x = train.stft_ragged(mix, row_lens)
        mark("stft_ragged")
        y = train.forward_train(model, x)
        mark("forward_train")
        x_time = train.IstftRaggedFunction.apply(y, row_lens)
        s = train.stft_ragged(speech, row_lens)
        losses, sdrs = train.TriLossRaggedFunction.apply(y, s, x_time, speech, lens, rows)
        mark("istft_ragged + stft_ragged + loss")
        losses.sum().backward()
        mark("backward")
        h1 = time.perf_counter()
        torch.cuda.synchronize()
        h2 = time.perf_counter()
        for p in model.parameters():
            p.grad = None
    say("# stages of (b), %d rows x %d frames, device time between events (the last of 3 runs); host: %.2f ms to enqueue, %.2f ms until the device is done"
        % (mix.shape[0], spec.n_frames(lens[0]), (h1 - h0) * 1e3, (h2 - h0) * 1e3))
    for (_, a), (name, b) in zip(marks, marks[1:]):
        say("#   %-36s %8.3f ms" % (name, a.elapsed_time(b)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
