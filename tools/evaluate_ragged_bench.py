#!/usr/bin/env python3
"""The batched validation pass against the loop it replaces, in one process on one GPU, inputs resident, after a warm-up of every shape:

  workload: 32 stereo (mixture, clean speech) pairs whose frame counts are spread evenly over 32 .. 126 (64 rows, 5 056 real row-frames)
  (a) one BSRNN.evaluate per pair               what validate.py does without --batch-rows: 32 calls of 2 rows
  (b) BSRNN.evaluate_many(pairs)                spec.ragged_buckets with the defaults (64 rows, padding share <= 0.25), one
                                                evaluate_ragged per bucket, the packing copies included

Both variants are synchronous (the metrics come back to the host), under the default range policy.  Each figure is the median over REPEATS
windows of a host clock around enough jobs to fill ~0.3 s; the two variants alternate inside every repeat.  The min .. max of the windows is
printed beside the median, with the padding share 1 - real row-frames / computed row-frames of (b).  Before anything is timed the two
results are compared pair by pair.

    python tools/evaluate_ragged_bench.py [--out profiles/evaluate_ragged.txt]
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
DB_KEYS = ("sdr", "input_sdr", "sisdr", "separation_db")


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

    frames = [int(round(T_LO + i * (T_HI - T_LO) / (N_CLIPS - 1))) for i in range(N_CLIPS)]
    order = np.random.RandomState(3).permutation(N_CLIPS)              # a validation set does not arrive sorted
    frames = [frames[i] for i in order]
    lens = [(t - 1) * HOP + 77 for t in frames]
    pairs = []
    for i, n in enumerate(lens):
        speech = weights.synth_waveform(CHANNELS, n, seed=140 + i, scale=0.07)
        mix = speech + weights.synth_waveform(CHANNELS, n, seed=40 + i, scale=0.05)
        pairs.append((torch.from_numpy(mix).cuda(), torch.from_numpy(speech).cuda()))
    real = sum(CHANNELS * t for t in frames)
    buckets = spec.ragged_buckets(frames, [CHANNELS] * N_CLIPS, 64, 0.25)
    computed_b = sum(CHANNELS * len(b) * max(frames[i] for i in b) for b in buckets)

    def job_a():
        return [model.evaluate(m, s) for m, s in pairs]

    def job_b():
        return model.evaluate_many(pairs)

    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# %d pairs x %d channels, frames %d .. %d (%d real row-frames); ms per job: median [min .. max] of %d windows of ~%.1f s"
        % (N_CLIPS, CHANNELS, min(frames), max(frames), real, REPEATS, WINDOW_S))
    say("# (b) buckets (pairs, rows x frames): %s" % ", ".join("%d: %d x %d" % (len(b), CHANNELS * len(b), max(frames[i] for i in b)) for b in buckets))

    # the same numbers, to rounding (kernels chosen for other row counts): before any timing
    ra, rb = job_a(), job_b()
    e_db = max(abs(x[k] - y[k]) for x, y in zip(ra, rb) for k in DB_KEYS)
    e_rel = max(abs(x[k] - y[k]) / abs(x[k]) for x, y in zip(ra, rb) for k in ("loss", "l1_time", "l1_re", "l1_im"))
    say("# largest |b - a|: %.3e dB on the decibel figures, %.3e relative on the L1 terms" % (e_db, e_rel))
    assert e_db < 2e-3 and e_rel < 2e-5, (e_db, e_rel)

    jobs = {"a": job_a, "b": job_b}
    n = {}
    for k, f in jobs.items():                 # warm-up, and how many jobs fill a window
        for _ in range(3):
            f()
        t0 = time.perf_counter()
        for _ in range(3):
            f()
        n[k] = max(3, int(WINDOW_S / max((time.perf_counter() - t0) / 3, 1e-6)))
    t = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, f in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n[k]):
                f()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / n[k] * 1e3)
    med = {k: float(np.median(v)) for k, v in t.items()}
    share = {"a": 0.0, "b": 1 - real / computed_b}
    calls = {"a": N_CLIPS, "b": len(buckets)}
    what = {"a": "evaluate per pair", "b": "evaluate_many"}
    say("%-24s %6s %30s %10s %16s %8s" % ("variant", "calls", "ms per job", "padding", "real Mrow-fr/s", "a / x"))
    for k in "ab":
        say("%-24s %6d %12.3f [%6.3f .. %6.3f] %10.3f %16.3f %8.2f" % ("(%s) %s" % (k, what[k]), calls[k], med[k], min(t[k]), max(t[k]), share[k],
                                                                      real / med[k] * 1e-3, med["a"] / med[k]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
