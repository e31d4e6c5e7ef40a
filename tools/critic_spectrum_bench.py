#!/usr/bin/env python3
"""Times the critic's 4096-point analysis (discriminator.critic_spectrum -> bsrnn_critic_spectrum, csrc/stft4096.hip) beside
torch.stft + torch.cat on the same device, at the critic's shortest input (R = 4, T = 601) and at a 60 s clip (R = 4, T = 2584).
Medians of `--reps` runs after `--warmup`, device events around each run, nothing else on the GPU.  Beside every figure the floor:
the bytes the call must move - the waveform in, the spectrum out - over HBM bandwidth (about 6.3 TB/s); the call itself also writes
and reads its frame-major records once (three times the spectrum's bytes in all), printed as a second floor.

    python tools/critic_spectrum_bench.py > profiles/critic_spectrum_bench.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechseparation_amd.discriminator import critic_spectrum, spectrum_layout       # noqa: E402

HBM_TBS = 6.3


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--frames", type=int, nargs="*", default=[601, 2584])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    win = torch.hann_window(4096, device=dev)
    print("critic_spectrum_bench: %s, medians of %d after %d warm-up runs; ms per call | floors at %.1f TB/s" % (
        torch.cuda.get_device_name(0), args.reps, args.warmup, HBM_TBS))
    for T in args.frames:
        R, n = args.rows, (T - 1) * 1024
        w = torch.randn(R, n, device=dev)
        g = spectrum_layout(R, n)
        assert g["T"] == T

        def stock():
            X = torch.stft(w * 0.5, n_fft=4096, hop_length=1024, window=win, return_complex=True)
            return torch.cat((X.real, X.imag), dim=1)
        ours = timed(lambda: critic_spectrum(w, 0.5), args.warmup, args.reps)
        ref = timed(stock, args.warmup, args.reps)
        err = float((critic_spectrum(w, 0.5) - stock()).abs().max())
        b_in, b_out = 4.0 * R * n, 4.0 * R * 4098 * T
        floor, floor3 = (b_in + b_out) / (HBM_TBS * 1e12) * 1e3, (b_in + 3 * b_out) / (HBM_TBS * 1e12) * 1e3
        print("\nR = %d, T = %d frames (n = %d): %.1f MB in, %.1f MB out; %d slabs of %d frames, %.1f MB of workspace" % (
            R, T, n, b_in * 1e-6, b_out * 1e-6, g["slabs"], g["frames_per_slab"], g["scratch_floats"] * 4e-6))
        print("  critic_spectrum      %8.3f ms | floor %.4f ms in + out (%.0f %% of it reached), %.4f ms with the records written and read" % (
            ours, floor, 100 * floor / ours, floor3))
        print("  torch.stft + cat     %8.3f ms   (max |difference| of the two results %.3e)" % (ref, err))


if __name__ == "__main__":
    main()
