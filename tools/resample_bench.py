#!/usr/bin/env python3
"""Sample-rate conversion on the device against its floor and against what it replaces, in one process on one GPU, after a warm-up of
every shape:

  workload: 64 rows x 10 s at 48 k -> 44.1 k, 44.1 k -> 48 k, 16 k -> 44.1 k and 192 k -> 44.1 k
  (k) bsrnn_resample into a preallocated result              one launch of resample_kernel, called through ctypes as a C host would
                                                             (BSRNN.resample adds its look at the model's parameters, tens of
                                                             microseconds of host time, to a call of this length)
  (c) a device-to-device copy with the same HBM traffic      the kernel reads R * n_in and writes R * n_out floats; a copy of
                                                             R * (n_in + n_out) / 2 floats reads and writes as many bytes: the floor
  (h) audio.resample on the host plus the upload             scipy resample_poly over the 64 rows in float64 on one thread, then
                                                             .cuda(): what a caller paid before

  and bsrnn.Resampler.process of one 1024-sample hop at 48 k -> 44.1 k for 2 and for 64 rows (a launch-bound call).

(k) and (c) alternate inside every repeat; each figure is the median over REPEATS windows of a host clock around enough calls to fill
~0.3 s, ending in a device synchronise, with the min .. max of the windows beside it.  (h) takes seconds per call and is timed
HOST_REPEATS times, one call each.  Before anything is timed the device result is compared with resample_poly of the float64 input.

    python tools/resample_bench.py [--out profiles/resample_bench.txt]
"""
import argparse
import ctypes
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, SECONDS = 64, 10
PAIRS = [(48000, 44100), (44100, 48000), (16000, 44100), (192000, 44100)]
REPEATS, HOST_REPEATS = 7, 3
WINDOW_S = 0.3


def windows(jobs, sync):
    """{name: [ms per call of each window]}: the jobs alternate inside every repeat."""
    n = {}
    for k, f in jobs.items():
        for _ in range(3):
            f()
        sync()
        t0 = time.perf_counter()
        for _ in range(5):
            f()
        sync()
        n[k] = max(5, int(WINDOW_S / max((time.perf_counter() - t0) / 5, 1e-7)))
    t = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, f in jobs.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(n[k]):
                f()
            sync()
            t[k].append((time.perf_counter() - t0) / n[k] * 1e3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scipy.signal import resample_poly
    from speechseparation_amd import _native, audio
    from speechseparation_amd.bsrnn import BSRNN, Resampler
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = BSRNN().eval().to("cuda:0")            # (the conversion needs a context, not trained weights)
    sync = torch.cuda.synchronize
    ctx = model._context(torch.device("cuda:0"))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    say("# %s, %s; %d rows x %d s; ms per call: median [min .. max] of %d windows of ~%.1f s (host path: %d single calls)"
        % (torch.cuda.get_device_name(0), torch.version.hip, ROWS, SECONDS, REPEATS, WINDOW_S, HOST_REPEATS))
    say("%-18s %9s %9s %5s %28s %28s %8s %9s %22s %8s" % ("pair", "n_in", "n_out", "L", "(k) resample ms", "(c) copy ms", "k / c", "GB/s (k)",
                                                         "(h) host + upload ms", "h / k"))
    for rate_in, rate_out in PAIRS:
        g = math.gcd(rate_in, rate_out)
        up, down = rate_out // g, rate_in // g
        half = 10 * max(up, down)
        L = half // up + (half + up - 1) // up + 1
        n_in = rate_in * SECONDS
        host = torch.from_numpy(0.1 * np.random.default_rng(1).standard_normal((ROWS, n_in)).astype(np.float32))
        x = host.cuda()
        out = model.resample(x, rate_in, rate_out)
        n_out = out.shape[1]
        ref = resample_poly(host[:2].numpy().astype(np.float64), up, down, axis=1)
        err = float(np.abs(out[:2].cpu().numpy() - ref).max())
        assert err < 1e-5, err
        half_traffic = ROWS * (n_in + n_out) // 2
        src, dst = torch.empty(half_traffic, device="cuda"), torch.empty(half_traffic, device="cuda")
        px, po = ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(out.data_ptr())

        def job_k():
            assert _native.lib.bsrnn_resample(ctx, px, n_in, po, n_out, ROWS, n_in, rate_in, rate_out, stream) == 0
        t = windows({"k": job_k, "c": lambda: dst.copy_(src)}, sync)
        th = []
        for _ in range(HOST_REPEATS):
            t0 = time.perf_counter()
            audio.resample(host, rate_in, rate_out).cuda()
            sync()
            th.append((time.perf_counter() - t0) * 1e3)
        k, c, h = float(np.median(t["k"])), float(np.median(t["c"])), float(np.median(th))
        say("%-18s %9d %9d %5d %10.4f [%7.4f .. %7.4f] %10.4f [%7.4f .. %7.4f] %8.2f %9.0f %10.1f [%8.1f] %8.0f" % (
            "%d -> %d" % (rate_in, rate_out), n_in, n_out, L, k, min(t["k"]), max(t["k"]), c, min(t["c"]), max(t["c"]), k / c,
            ROWS * (n_in + n_out) * 4 / k * 1e-6, h, min(th), h / k))
        say("#   max |device - resample_poly(float64)| over two rows: %.2e" % err)
        del x, out, src, dst
    for rows in (2, 64):
        rs = Resampler(model, rows, 48000, 44100)
        hop = torch.from_numpy(0.1 * np.random.default_rng(2).standard_normal((rows, 1024)).astype(np.float32)).cuda()
        t = windows({"p": lambda: rs.process(hop)}, sync)["p"]
        say("Resampler.process, one 1024-sample hop, %2d rows, 48000 -> 44100: %.4f ms per call [%.4f .. %.4f] (result tensor allocated per call)"
            % (rows, float(np.median(t)), min(t), max(t)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
