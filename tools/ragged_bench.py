#!/usr/bin/env python3
"""Ragged batches against the loop they replace, in one process on one GPU, inputs resident, deferred range policy, after a warm-up
of every shape:

  workload: 32 stereo clips whose frame counts are spread evenly over 32 .. 126 (64 rows, 5 056 real row-frames)
  (a) one BSRNN.separate per clip               what a caller had before: 32 calls of 2 rows
  (b) BSRNN.separate_many(clips)                spec.ragged_buckets with the defaults (64 rows, padding share <= 0.25), one
                                                separate_ragged per bucket, the packing copies and the result slices included
  (c) one BSRNN.separate_ragged over all 64 rows, from a packed buffer (the packing not included)

Each figure is the median over REPEATS windows of a host clock around enough jobs to fill ~0.3 s, ending in a device synchronise; the
three variants alternate inside every repeat.  The min .. max of the windows is printed beside the median, with the padding share
1 - real row-frames / computed row-frames of (b) and (c).  Before anything is timed the three results are compared clip by clip.

    python tools/ragged_bench.py [--out profiles/ragged_batch.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_CLIPS, CHANNELS = 32, 2
T_LO, T_HI = 32, 126
REPEATS = 7
WINDOW_S = 0.3
HOP = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speechseparation_amd import _native, spec, weights
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = weights.synth_state_dict(None, seed=0)
    model = BSRNN().eval()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to("cuda:0")
    model.set_range_policy("deferred")

    frames = [int(round(T_LO + i * (T_HI - T_LO) / (N_CLIPS - 1))) for i in range(N_CLIPS)]
    order = np.random.RandomState(3).permutation(N_CLIPS)              # a queue does not arrive sorted
    frames = [frames[i] for i in order]
    lens = [(t - 1) * HOP + 77 for t in frames]
    clips = [torch.from_numpy(weights.synth_waveform(CHANNELS, n, seed=40 + i)).cuda() for i, n in enumerate(lens)]
    packed = torch.zeros((N_CLIPS * CHANNELS, max(lens)), device="cuda")
    for i, c in enumerate(clips):
        packed[CHANNELS * i:CHANNELS * (i + 1), :lens[i]] = c
    row_lens = [n for n in lens for _ in range(CHANNELS)]
    real = sum(CHANNELS * t for t in frames)
    buckets = spec.ragged_buckets(frames, [CHANNELS] * N_CLIPS, 64, 0.25)
    computed_b = sum(CHANNELS * len(b) * max(frames[i] for i in b) for b in buckets)
    computed_c = N_CLIPS * CHANNELS * max(frames)

    def job_a():
        return [model.separate(c) for c in clips]

    def job_b():
        return model.separate_many(clips)

    def job_c():
        return model.separate_ragged(packed, row_lens)

    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# %d clips x %d channels, frames %d .. %d (%d real row-frames); ms per job: median [min .. max] of %d windows of ~%.1f s"
        % (N_CLIPS, CHANNELS, min(frames), max(frames), real, REPEATS, WINDOW_S))
    say("# (b) buckets (clips, rows x frames): %s" % ", ".join("%d: %d x %d" % (len(b), CHANNELS * len(b), max(frames[i] for i in b)) for b in buckets))

    # the same samples, to rounding (kernels chosen for other row counts): before any timing
    ra, rb, rc = job_a(), job_b(), job_c()
    model.sync()
    kept = [(n // HOP) * HOP for n in lens]
    e_b = max(float((x - y).abs().max()) for x, y in zip(ra, rb))
    e_c = max(float((ra[i] - rc[CHANNELS * i:CHANNELS * (i + 1), :kept[i]]).abs().max()) for i in range(N_CLIPS))
    peak = max(float(x.abs().max()) for x in ra)
    say("# max|b - a| %.3e, max|c - a| %.3e at a peak of %.3f" % (e_b, e_c, peak))
    assert e_b < 3e-5 and e_c < 3e-5, (e_b, e_c)

    jobs = {"a": job_a, "b": job_b, "c": job_c}
    n = {}
    for k, f in jobs.items():                 # warm-up, and how many jobs fill a window
        for _ in range(3):
            f()
        model.sync()
        t0 = time.perf_counter()
        for _ in range(3):
            f()
        model.sync()
        n[k] = max(3, int(WINDOW_S / max((time.perf_counter() - t0) / 3, 1e-6)))
    t = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, f in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n[k]):
                f()
            model.sync()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / n[k] * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    share = {"a": 0.0, "b": 1 - real / computed_b, "c": 1 - real / computed_c}
    calls = {"a": N_CLIPS, "b": len(buckets), "c": 1}
    what = {"a": "separate per clip", "b": "separate_many", "c": "one separate_ragged"}
    say("%-24s %6s %30s %10s %16s %8s" % ("variant", "calls", "ms per job", "padding", "real Mrow-fr/s", "a / x"))
    for k in "abc":
        say("%-24s %6d %12.3f [%6.3f .. %6.3f] %10.3f %16.3f %8.2f" % ("(%s) %s" % (k, what[k]), calls[k], med[k], min(t[k]), max(t[k]), share[k],
                                                                      real / med[k] * 1e-3, med["a"] / med[k]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
