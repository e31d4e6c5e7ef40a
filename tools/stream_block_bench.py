#!/usr/bin/env python3
"""Block streaming against its alternatives, in one process on one GPU, inputs resident, deferred range policy, after reserve:

  (a) bsrnn_stream_process(L)                   one call for L hops
  (b) L calls of bsrnn_stream_step              the same job hop by hop
  (c) bsrnn_forward_chunk(C, L)                 the same model on a resident spectrum (two layout kernels instead of two FFT kernels)

Each figure is the median over REPEATS windows of a host clock around enough jobs to fill ~0.2 s, ending in a device synchronise;
the three variants alternate inside every repeat.  The min .. max of the windows is printed beside the median.  The two block DSP
kernels' own durations come from the stream_dsp stage bracket (events around each launch; both kernels share the bracket, so the
figure is analysis + synthesis per call), in a pass of its own, beside the layout bracket of (c) at the same shape and the offline
stft / istft brackets at 64 rows x 126 frames.

    python tools/stream_block_bench.py [--out profiles/stream_block.txt]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(2, 1), (2, 2), (2, 8), (2, 43), (2, 256), (64, 1), (64, 11), (64, 256)]
REPEATS = 7
WINDOW_S = 0.2
HOP = 1024
DSP_BYTES = 2 * (HOP * 4 + 2050 * 4)         # per row-frame, analysis + synthesis: 4 KiB of samples and 8.2 KB of spectrum each way


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import BSRNN, StreamingSeparator
    lib, check = _native.lib, _native.check
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
    dev = torch.device("cuda", 0)
    ctx = model._context(dev)
    K = len(model.band_widths)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    one = ctypes.c_float(1.0)
    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# us per job of L hops: median [min .. max] of %d windows of ~%.1f s; a = stream_process(L), b = L x stream_step, c = forward_chunk(C, L)"
        % (REPEATS, WINDOW_S))
    say("%4s %4s %28s %28s %28s %8s %8s %14s" % ("C", "L", "a us", "b us", "c us", "b/a", "a/c", "a Mrow-frames/s"))
    dsp = {}
    for C, L in SHAPES:
        st = StreamingSeparator(model, channels=C, device=dev)
        st.reserve(L)
        wave = torch.from_numpy(weights.synth_waveform(C, L * HOP, seed=5)).cuda()
        out = torch.empty_like(wave)
        hops = [wave[:, l * HOP:(l + 1) * HOP].contiguous() for l in range(L)]
        hop_out = torch.empty((C, HOP), device="cuda")
        x = torch.from_numpy(weights.synth_tensor((C, 2050, L), seed=6, scale=1.0)).cuda()
        y = torch.empty_like(x)
        s_in = torch.zeros((4, 2, C * K, 64), device="cuda")
        s_out = torch.empty_like(s_in)

        def job_a():
            check(lib.bsrnn_stream_process(st._h, ptr(wave), ptr(out), L, one, None))

        def job_b():
            for l in range(L):
                check(lib.bsrnn_stream_step(st._h, ptr(hops[l]), ptr(hop_out), one, None))

        def job_c():
            check(lib.bsrnn_forward_chunk(ctx, ptr(x), ptr(s_in), ptr(y), ptr(s_out), C, L, None))

        jobs = {"a": job_a, "b": job_b, "c": job_c}
        n = {}
        for k, f in jobs.items():                 # warm-up, and how many jobs fill a window
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            n[k] = max(3, int(WINDOW_S / max((time.perf_counter() - t0) / 3, 1e-6)))
        t = {k: [] for k in jobs}
        for _ in range(REPEATS):
            for k, f in jobs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n[k]):
                    f()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / n[k] * 1e6)
        med = {k: float(np.median(v)) for k, v in t.items()}
        cell = lambda k: "%9.1f [%8.1f .. %8.1f]" % (med[k], min(t[k]), max(t[k]))
        say("%4d %4d %28s %28s %28s %8.2f %8.3f %14.3f" % (C, L, cell("a"), cell("b"), cell("c"), med["b"] / med["a"], med["a"] / med["c"],
                                                          C * L / med["a"]))
        # the DSP kernels' own time: the stream_dsp bracket only, in a pass of its own
        if L >= 2:
            model.set_profiling(["stream_dsp"])
            model.stage_times(reset=True)
            reps = 20
            for _ in range(reps):
                job_a()
            ms, cnt = model.stage_times(reset=True)["stream_dsp"]
            model.set_profiling(False)
            # ... and what (c) runs in their place: the two layout kernels, from the layout bracket
            model.set_profiling(["layout"])
            model.stage_times(reset=True)
            for _ in range(reps):
                job_c()
            lms, _ = model.stage_times(reset=True)["layout"]
            model.set_profiling(False)
            dsp[(C, L)] = (ms * 1e3 / reps, cnt // reps, lms * 1e3 / reps)
        model.sync()
        del st
    say("")
    say("# stream_dsp bracket per block call (analysis + synthesis kernels, %d B per row-frame between them)" % DSP_BYTES)
    for (C, L), (us, launches, lay) in dsp.items():
        say("C %3d L %3d: %8.1f us in %d launches, %7.1f GB/s   (layout bracket of c: %6.1f us)" % (C, L, us, launches, C * L * DSP_BYTES / us * 1e-3, lay))
    # the offline pair at the benchmark's size, from its own brackets
    R, T = 64, 126
    w = torch.from_numpy(weights.synth_waveform(R, (T - 1) * HOP + 1, seed=7)).cuda()
    for _ in range(3):
        model.separate(w)
    model.set_profiling(["stft", "istft"])
    model.stage_times(reset=True)
    reps = 20
    for _ in range(reps):
        model.separate(w)
    tm = model.stage_times(reset=True)
    model.set_profiling(False)
    a_us, s_us = tm["stft"][0] * 1e3 / reps, tm["istft"][0] * 1e3 / reps
    say("offline at %d x %d: stft %.1f us, istft %.1f us, together %.1f GB/s on the same %d B per row-frame"
        % (R, T, a_us, s_us, R * T * DSP_BYTES / (a_us + s_us) * 1e-3, DSP_BYTES))
    model.sync()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
