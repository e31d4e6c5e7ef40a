#!/usr/bin/env python3
"""The long FIR convolution on the device against what the reference runs and against torch's own FFT, in one process on one GPU, after a
warm-up of every shape:

  workload: 64 rows x 8 s at 44.1 kHz under a room impulse response of 0.5 s (22050 taps) and of 1 s (44100 taps)
  (k) bsrnn_convolve_ragged into a preallocated result       three launches (analysis, multiply-accumulate, synthesis), called through
                                                             ctypes as a C host would
  (f) torch's one-shot FFT convolution of the padded rows    irfft(rfft(x, N) * G, N)[shift : shift + n], N = 2^19 for both, G = the
                                                             filter's spectrum computed once outside the timed region (as the bank's is)
  (d) F.conv1d(x, h, padding='same') on the same device      the call the reference makes (m_dataset.py:110), here once for all 64 rows

(k) and (f) alternate inside every repeat; each figure is the median over REPEATS windows of a host clock around enough calls to fill
~0.3 s, ending in a device synchronise, with the min .. max of the windows beside it.  (d) is timed DIRECT_REPEATS times, one call each,
after one untimed call (its first call chooses and builds the convolution kernel).  Before anything is timed the three results are compared.
The tool fails if (k) is not faster than (d) at the 0.5 s response.

    python tools/convolve_bench.py [--out profiles/convolve_bench.txt] [--skip-direct]

--stream measures the streaming form (bsrnn_fir_stream_*) instead: 64 live rows, one hop of 1024 samples per row and tick, in a steady
state (every row has taken more hops than the filter has partitions), under the same two responses:

  (s) bsrnn_fir_stream_process, one call per tick                 one launch, a workgroup per row
  (w) what a user had before: bsrnn_convolve_ragged per tick      over the last k - 1 + 1024 samples of every row (P + 1 analysis transforms
                                                                  and a full multiply-accumulate per row, and not the one-shot's bits)
  (o) the one-shot's cost per hop                                 bsrnn_convolve_ragged of the 8 s rows, divided by their 344.5 hops

    python tools/convolve_bench.py --stream [--out profiles/convolve_stream_bench.txt]
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ROWS, SECONDS, RATE = 64, 8, 44100
TAPS = [22050, 44100]
REPEATS, DIRECT_REPEATS = 7, 3
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


def stream_main(args):
    from speechseparation_amd import _native
    from speechseparation_amd.augment import FirBank, FirStream
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    lib = _native.lib
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    model = BSRNN().eval().to("cuda:0")
    sync = torch.cuda.synchronize
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = RATE * SECONDS
    hops = n / 1024.0
    res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True).stdout
    say("# %s, %s; %d rows, one hop of 1024 samples per row and tick; ms per tick: median [min .. max] of %d windows of ~%.1f s"
        % (torch.cuda.get_device_name(0), torch.version.hip, ROWS, REPEATS, WINDOW_S))
    for ln in res.splitlines():
        if "fir_stream" in ln:
            say("#   " + " ".join(ln.split()))
    say("%8s %4s %30s %34s %8s %26s %8s" % ("taps", "P", "(s) fir_stream_process ms", "(w) convolve_ragged, window ms", "s / w", "(o) one-shot ms per hop", "s / o"))
    rng = np.random.default_rng(1)
    x = torch.from_numpy((0.1 * rng.standard_normal((ROWS, n))).astype(np.float32)).cuda()
    out = torch.empty_like(x)
    lens, filt = (ctypes.c_int64 * ROWS)(*[n] * ROWS), (ctypes.c_int32 * ROWS)(*[0] * ROWS)
    hop_in = (ctypes.c_int64 * ROWS)(*[1024] * ROWS)
    hop_out = (ctypes.c_int64 * ROWS)()
    ok = True
    for k in TAPS:
        h = (rng.standard_normal(k) * np.exp(-5.0 * np.arange(k) / k)).astype(np.float32)
        bank = FirBank(model, [h])
        P = -(-k // 1024)
        st = FirStream(bank, ROWS)
        st.assign(range(ROWS), 0)
        tick_out = torch.empty((ROWS, 1024), device="cuda")
        at = [0]

        def job_s():
            a = at[0] % (n // 1024)                 # the hop the rows bring this tick, cycling through x
            at[0] += 1
            assert lib.bsrnn_fir_stream_process(st._h, ctypes.c_void_p(x.data_ptr() + 4 * 1024 * a), n, hop_in, ctypes.c_void_p(tick_out.data_ptr()),
                                                1024, hop_out, stream) == 0
        wlen = k - 1 + 1024
        wlens = (ctypes.c_int64 * ROWS)(*[wlen] * ROWS)
        wout = torch.empty((ROWS, wlen), device="cuda")

        def job_w():
            assert lib.bsrnn_convolve_ragged(bank._h, ctypes.c_void_p(x.data_ptr()), n, wlens, filt, ctypes.c_void_p(wout.data_ptr()), wlen, ROWS, stream) == 0

        def job_o():
            assert lib.bsrnn_convolve_ragged(bank._h, ctypes.c_void_p(x.data_ptr()), n, lens, filt, ctypes.c_void_p(out.data_ptr()), n, ROWS, stream) == 0
        # the stream against the one-shot before anything is timed: the first hops of the rows, bit for bit; this is also the warm-up
        # into the steady state (every partition has a frame)
        job_o()
        got = []
        for _ in range(P + 4):
            job_s()
            got.append(tick_out[:, :int(hop_out[0])].clone())
        got = torch.cat(got, dim=1)
        assert got.shape[1] == (P + 4) * 1024 - k // 2 and torch.equal(got, out[:, :got.shape[1]]), "the stream is not the one-shot"
        t = windows({"s": job_s, "w": job_w, "o": job_o}, sync)
        ms, mw = float(np.median(t["s"])), float(np.median(t["w"]))
        to = [v / hops for v in t["o"]]
        mo = float(np.median(to))
        say("%8d %4d %12.4f [%7.4f .. %7.4f] %16.4f [%7.4f .. %7.4f] %8.2f %12.5f [%7.5f .. %7.5f] %8.1f" % (
            k, P, ms, min(t["s"]), max(t["s"]), mw, min(t["w"]), max(t["w"]), ms / mw, mo, min(to), max(to), ms / mo))
        ok = ok and ms < mw
        del st, bank
    say("# expectation: a tick (s) costs less than the windowed one-shot call (w): %s" % ("confirmed" if ok else "NOT CONFIRMED"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-direct", action="store_true", help="leave (d) out (and with it the gate)")
    ap.add_argument("--stream", action="store_true", help="measure the streaming form (bsrnn_fir_stream_*) instead")
    args = ap.parse_args()
    if args.stream:
        return stream_main(args)
    from speechseparation_amd import _native
    from speechseparation_amd.augment import FirBank
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    model = BSRNN().eval().to("cuda:0")            # (the convolution needs a context, not trained weights)
    sync = torch.cuda.synchronize
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = RATE * SECONDS
    res = subprocess.run([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py")], capture_output=True, text=True).stdout
    say("# %s, %s; %d rows x %d s at %d Hz; ms per call: median [min .. max] of %d windows of ~%.1f s ((d): %d single calls)"
        % (torch.cuda.get_device_name(0), torch.version.hip, ROWS, SECONDS, RATE, REPEATS, WINDOW_S, DIRECT_REPEATS))
    say("# library: %s" % os.path.relpath(_native.LIB_PATH, REPO))
    in_tree = os.path.realpath(_native.LIB_PATH) == os.path.realpath(os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so"))
    for ln in res.splitlines():                    # (kernel_resources.py reads the in-tree library)
        if "fir_" in ln and in_tree:
            say("#   " + " ".join(ln.split()))
    say("%8s %4s %30s %30s %8s %26s %8s" % ("taps", "P", "(k) convolve_ragged ms", "(f) torch.fft one-shot ms", "k / f", "(d) F.conv1d ms", "d / k"))
    rng = np.random.default_rng(1)
    x = torch.from_numpy((0.1 * rng.standard_normal((ROWS, n))).astype(np.float32)).cuda()
    out = torch.empty_like(x)
    lens, filt = (ctypes.c_int64 * ROWS)(*[n] * ROWS), (ctypes.c_int32 * ROWS)(*[0] * ROWS)
    gate = None
    for k in TAPS:
        h = (rng.standard_normal(k) * np.exp(-5.0 * np.arange(k) / k)).astype(np.float32)
        bank = FirBank(model, [h])
        hd = torch.from_numpy(h).cuda()
        N = 1 << int(np.ceil(np.log2(n + k - 1)))
        G = torch.fft.rfft(hd.flip(0), n=N)
        shift = k // 2

        def job_k():
            assert _native.lib.bsrnn_convolve_ragged(bank._h, ctypes.c_void_p(x.data_ptr()), n, lens, filt, ctypes.c_void_p(out.data_ptr()), n,
                                                     ROWS, stream) == 0

        def job_f():
            return torch.fft.irfft(torch.fft.rfft(x, n=N, dim=1) * G, n=N, dim=1)[:, shift:shift + n]

        def job_d():
            return F.conv1d(x.reshape(ROWS, 1, n), hd.reshape(1, 1, k), padding="same").reshape(ROWS, n)
        job_k()
        yf = job_f()
        err_f = float((out - yf).abs().max() / yf.abs().max())
        assert err_f < 1e-5, err_f
        t = windows({"k": job_k, "f": job_f}, sync)
        mk, mf = float(np.median(t["k"])), float(np.median(t["f"]))
        td, err_d = [], float("nan")
        if not args.skip_direct:
            yd = job_d()
            sync()
            err_d = float((out - yd).abs().max() / yd.abs().max())
            for _ in range(DIRECT_REPEATS):
                sync()
                t0 = time.perf_counter()
                job_d()
                sync()
                td.append((time.perf_counter() - t0) * 1e3)
            del yd
        md = float(np.median(td)) if td else float("nan")
        say("%8d %4d %12.4f [%7.4f .. %7.4f] %12.4f [%7.4f .. %7.4f] %8.2f %12.2f [%10.2f] %8.1f" % (
            k, -(-k // 1024), mk, min(t["k"]), max(t["k"]), mf, min(t["f"]), max(t["f"]), mk / mf, md, min(td) if td else float("nan"), md / mk))
        say("#   max |k - f| / max |f| = %.2e, max |k - d| / max |d| = %.2e" % (err_f, err_d))
        if k == TAPS[0] and td:
            gate = (mk, md)
        del bank, G, yf
    if gate:
        say("# gate: (k) %.4f ms < (d) %.2f ms at %d taps: %s" % (gate[0], gate[1], TAPS[0], "met" if gate[0] < gate[1] else "MISSED"))
        assert gate[0] < gate[1], gate


if __name__ == "__main__":
    main()
