#!/usr/bin/env python3
"""Long-form separation against the one-shot call, in one process on one GPU: a clip of R rows (default 2 rows, 10 minutes at
44.1 kHz) through

  (a) BSRNN.separate                               the whole clip in one call: workspace of R * T frame rows
  (b) BSRNN.separate_long(seg_frames), device      the clip resident on the device, segments of seg_frames frames
  (c) BSRNN.separate_long(seg_frames), host        the clip in host memory, staged through pinned windows beside the kernels

for seg_frames in 64, 128, 256, 512, 1024.  Every variant is run on a fresh model (its own native context), so the workspace figure
is that variant's alone; it is warmed up twice and then timed REPEATS times with a host clock around the call ending in a device
synchronise; the figure is the median, min .. max beside it.  Variants alternate inside every repeat.  Both range policies are
measured: under 'exact' (the default, what infer.py runs) the library waits after every segment, under 'deferred' no segment waits.
(a) and (b) include no transfer of the clip; (c) includes both directions, as (a) would have to add them for a file.

    python tools/long_separate_bench.py [--minutes 10] [--rows 2] [--out profiles/long_separate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SEGS = (64, 128, 256, 512, 1024)
REPEATS = 5
HOP = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    R, n = args.rows, int(args.minutes * 60 * args.rate)
    T = 1 + n // HOP
    sd = weights.synth_state_dict(None, seed=0)
    host = torch.from_numpy(weights.synth_waveform(R, n, seed=5))
    dev = host.cuda()
    out_dev = torch.empty((R, (T - 1) * HOP), device="cuda")
    out_host = torch.empty((R, (T - 1) * HOP))

    def fresh(policy):
        m = BSRNN().eval()
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m = m.to("cuda:0")
        m.set_range_policy(policy)
        return m

    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# R = %d rows, n = %d samples (%.1f min at %d Hz), T = %d frames, %d row-frames; ms per clip: median [min .. max] of %d runs"
        % (R, n, args.minutes, args.rate, T, R * T, REPEATS))
    for policy in ("exact", "deferred"):
        variants = [("separate", None, fresh(policy), lambda m: m.separate(dev, out=out_dev))]
        for seg in SEGS:
            variants.append(("long dev", seg, fresh(policy), lambda m, seg=seg: m.separate_long(dev, seg, out=out_dev)))
            variants.append(("long host", seg, fresh(policy), lambda m, seg=seg: m.separate_long(host, seg, out=out_host)))
        for _, _, m, f in variants:
            for _ in range(2):
                f(m)
            m.sync()
        torch.cuda.synchronize()
        t = [[] for _ in variants]
        for _ in range(REPEATS):
            for i, (_, _, m, f) in enumerate(variants):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f(m)
                torch.cuda.synchronize()
                t[i].append((time.perf_counter() - t0) * 1e3)
        say("")
        say("# range policy '%s'" % policy)
        say("%-10s %6s %30s %14s %16s %10s" % ("variant", "seg", "ms per clip", "workspace rows", "Mrow-frames/s", "vs (a)"))
        base = float(np.median(t[0]))
        for i, (name, seg, m, _) in enumerate(variants):
            med = float(np.median(t[i]))
            say("%-10s %6s %12.2f [%7.2f .. %7.2f] %14d %16.4f %10.3f" % (name, "-" if seg is None else seg, med, min(t[i]), max(t[i]),
                                                                          m.workspace_rows(), R * T / med * 1e-3, med / base))
        for _, _, m, _ in variants:
            m.sync()
        del variants
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
