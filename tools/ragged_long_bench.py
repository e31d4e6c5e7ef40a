#!/usr/bin/env python3
"""Long AND unequal clips: ragged long-form separation against the two ways a caller had before, in one process on one GPU, inputs
resident, deferred range policy, after a warm-up of every shape:

  workload: 32 stereo clips whose frame counts are spread evenly over 64 .. 2048 (64 rows), in a shuffled order
  (a) one BSRNN.separate_long per clip           32 calls of 2 rows, segments of SEG frames: bounded memory, launch-bound
  (b) BSRNN.separate_many(clips)                 spec.ragged_buckets with the defaults (64 rows, padding share <= 0.25), one
                                                 separate_ragged per bucket on the rectangle rows x longest clip: workspace of rows x Tmax
  (c) BSRNN.separate_many_long(clips)            spec.long_buckets (64 rows, no padding cap), one separate_long_ragged per bucket,
                                                 segments of SEG frames on the alive prefix of the rows: workspace of rows x SEG
  (b) and (c) include the packing copies and the result slices.

Each figure is the median over REPEATS windows of a host clock around enough jobs to fill ~0.3 s (at least two), ending in a device
synchronise; the three variants alternate inside every repeat.  The min .. max of the windows is printed beside the median, with the
frame rows (rows x frames) each variant hands to the model - for (c) as bsrnn_debug_counter(4) counts them - and the workspace rows of
each variant's own context afterwards.  Before anything is timed the three results are compared clip by clip.

    python tools/ragged_long_bench.py [--segment-frames 256] [--out profiles/ragged_long.txt]
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
T_LO, T_HI = 64, 2048
REPEATS = 7
WINDOW_S = 0.3
HOP = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segment-frames", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    seg = args.segment_frames
    from speechseparation_amd import _native, spec, weights
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd = weights.synth_state_dict(None, seed=0)

    def fresh():            # a context per variant: the workspace is grow-only, and each variant's own is what is reported
        m = BSRNN().eval()
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m = m.to("cuda:0")
        m.set_range_policy("deferred")
        return m
    models = {k: fresh() for k in "abc"}

    frames = [int(round(T_LO + i * (T_HI - T_LO) / (N_CLIPS - 1))) for i in range(N_CLIPS)]
    order = np.random.RandomState(3).permutation(N_CLIPS)              # a directory of recordings does not arrive sorted
    frames = [frames[i] for i in order]
    lens = [(t - 1) * HOP + 77 for t in frames]
    clips = [torch.from_numpy(weights.synth_waveform(CHANNELS, n, seed=40 + i)).cuda() for i, n in enumerate(lens)]
    real = sum(CHANNELS * t for t in frames)
    rows_of = [CHANNELS] * N_CLIPS
    buckets_b = spec.ragged_buckets(frames, rows_of, 64, 0.25)
    buckets_c = spec.long_buckets(frames, rows_of, 64)
    run_a = sum(CHANNELS * t for t in frames)
    run_b = sum(CHANNELS * len(b) * max(frames[i] for i in b) for b in buckets_b)
    run_c = sum(spec.long_plan([frames[i] for i in b for _ in range(CHANNELS)], seg)[1] for b in buckets_c)

    jobs = {"a": lambda: [models["a"].separate_long(c, seg) for c in clips],
            "b": lambda: models["b"].separate_many(clips),
            "c": lambda: models["c"].separate_many_long(clips, segment_frames=seg)}

    def sync():
        for m in models.values():
            m.sync()
        torch.cuda.synchronize()

    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# %d clips x %d channels, frames %d .. %d (%d real frame rows), segments of %d frames; ms per job: median [min .. max] of %d windows of ~%.1f s"
        % (N_CLIPS, CHANNELS, min(frames), max(frames), real, seg, REPEATS, WINDOW_S))
    say("# (b) buckets (clips, rows x frames): %s" % ", ".join("%d: %d x %d" % (len(b), CHANNELS * len(b), max(frames[i] for i in b)) for b in buckets_b))
    say("# (c) buckets (clips, rows, alive prefixes): %s" % "; ".join(
        "%d: %d, %s" % (len(b), CHANNELS * len(b), spec.long_plan([frames[i] for i in b for _ in range(CHANNELS)], seg)[0]) for b in buckets_c))

    # the same samples, to rounding (kernels chosen for other call shapes): before any timing
    ra, rb = jobs["a"](), jobs["b"]()
    before = _native.lib.bsrnn_debug_counter(4)
    rc = jobs["c"]()
    sync()
    counted_c = _native.lib.bsrnn_debug_counter(4) - before
    e_b = max(float((x - y).abs().max()) for x, y in zip(ra, rb))
    e_c = max(float((x - y).abs().max()) for x, y in zip(ra, rc))
    peak = max(float(x.abs().max()) for x in ra)
    say("# max|b - a| %.3e, max|c - a| %.3e at a peak of %.3f; frame rows (c) handed to the model: %d counted, %d planned" % (e_b, e_c, peak, counted_c, run_c))
    assert e_b < 3e-5 and e_c < 3e-5, (e_b, e_c)
    assert counted_c == run_c
    del ra, rb, rc

    n = {}
    for k, f in jobs.items():                 # warm-up, and how many jobs fill a window
        f()
        sync()
        t0 = time.perf_counter()
        for _ in range(2):
            f()
        sync()
        n[k] = max(2, int(WINDOW_S / max((time.perf_counter() - t0) / 2, 1e-6)))
    t = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, f in jobs.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(n[k]):
                f()
            sync()
            t[k].append((time.perf_counter() - t0) / n[k] * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    ran = {"a": run_a, "b": run_b, "c": run_c}
    calls = {"a": N_CLIPS, "b": len(buckets_b), "c": len(buckets_c)}
    what = {"a": "separate_long per clip", "b": "separate_many", "c": "separate_many_long"}
    say("%-28s %6s %6s %32s %12s %10s %16s %14s" % ("variant", "calls", "jobs", "ms per job", "frame rows", "/ real", "real Mrow-fr/s", "workspace rows"))
    for k in "abc":
        say("%-28s %6d %6d %12.3f [%7.3f .. %7.3f] %12d %10.3f %16.3f %14d" % (
            "(%s) %s" % (k, what[k]), calls[k], n[k], med[k], min(t[k]), max(t[k]), ran[k], ran[k] / real, real / med[k] * 1e-3, models[k].workspace_rows()))
    say("# (c) against (a): %.2fx, against (b): %.2fx (ms per job, medians)" % (med["a"] / med["c"], med["b"] / med["c"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
