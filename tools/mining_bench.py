#!/usr/bin/env python3
"""The section mining on the device, measured in one run on one GPU at the size a user mines at: 64 rows x 60 s at 44.1 kHz.

  (a) bsrnn_hop_activity alone, device-side: hip events around CALLS back-to-back calls (through ctypes, as a C host would make them) into
      a preallocated result, after a warm-up; median [min .. max] over REPEATS such windows, in us per call and in GB/s of the 8 bytes per
      sample the kernel has to read.
  (b) the same kernel and metric_time_ragged_kernel - the project's existing reduction over the same kind of data (three signals, 12 bytes
      per sample; bsrnn_evaluate_ragged launches it) - by kernel time: a child process of this tool under `rocprofv3 --kernel-trace
      --stats` calls both on the same buffers (the mixture, and the estimate in the place of the clean signal).  The evaluate call
      separates its whole rectangle at once, so this part runs on 16 of the rows (16 x 60 s: 0.34 GB and 0.51 GB read, more than the
      256 MB of last-level cache); if the call cannot be made the line says so.  It runs last and nothing else depends on it.
  (c) `mining.mine` end to end beside `BSRNN.separate_many_long` alone on the same 64 clips (already on the device), alternating: a host
      clock around calls that end in a device synchronise.

    python tools/mining_bench.py [--out profiles/mining_bench.txt] [--skip-trace] [--rows 64 --seconds 60]
"""
import argparse
import csv
import ctypes
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RATE, HOP = 44100, 1024
CALLS, REPEATS, E2E_REPEATS, PROBE_CALLS = 50, 15, 5, 30
TRACE_ROWS, TRACE_TIMEOUT_S = 16, 300


def buffers(rows, seconds):
    import torch
    n = RATE * seconds
    g = torch.Generator(device="cuda").manual_seed(1)
    mix = 0.1 * torch.randn((rows, n), device="cuda", generator=g)
    return mix, n


def probe(rows, seconds):
    """The traced child: warm-up, then PROBE_CALLS activity launches and two evaluate calls on the same buffers."""
    import torch
    from speechseparation_amd import mining
    from speechseparation_amd.bsrnn import BSRNN
    model = BSRNN().eval().to("cuda:0")
    mix, n = buffers(rows, seconds)
    est = (0.5 * mix[:, :n // HOP * HOP]).contiguous()
    out = torch.empty((rows, n // HOP, 2), device="cuda", dtype=torch.float64)
    for _ in range(3 + PROBE_CALLS):
        mining.hop_activity(model, mix, est, out=out)
    torch.cuda.synchronize()
    speech = torch.zeros_like(mix)
    speech[:, :est.shape[1]] = est
    try:
        for _ in range(2):
            model.evaluate_ragged(mix, speech, [n] * rows)
    except Exception as e:                         # (the comparison is reported as not made; the activity launches are in the trace)
        print("evaluate_ragged at this size: %s" % e, flush=True)
    torch.cuda.synchronize()


def traced(rows, seconds, say):
    d = tempfile.mkdtemp(prefix="mining_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--probe", "--rows", str(rows), "--seconds", str(seconds)]
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
        try:
            stdout, _ = proc.communicate(timeout=TRACE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)            # the profiler and the process under it
            proc.wait()
            say("# (b) kernel trace: not measured (the traced process did not end within %d s)" % TRACE_TIMEOUT_S)
            sys.exit(124)
        res = subprocess.CompletedProcess(cmd, proc.returncode, stdout)
        files = glob.glob(os.path.join(d, "*", "*kernel_stats.csv"))
        if res.returncode != 0 or not files:
            say("# (b) kernel trace: not measured (rocprofv3 exit %d)" % res.returncode)
            for ln in res.stdout.splitlines()[-5:]:
                say("#     " + ln)
            return
        for ln in res.stdout.splitlines():
            if ln.startswith("evaluate_ragged at this size"):
                say("# (b) " + ln)
        samples = rows * (RATE * seconds // HOP) * HOP
        say("# (b) kernel times from the trace of a child process, %d rows x %d s:" % (rows, seconds))
        found = {}
        for r in csv.DictReader(open(files[0])):
            for key, bytes_per_sample in (("hop_activity_kernel", 8), ("metric_time_ragged_kernel", 12)):
                if key in r["Name"]:
                    found[key] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, bytes_per_sample)
        for key in ("hop_activity_kernel", "metric_time_ragged_kernel"):
            if key in found:
                calls, us, b = found[key]
                say("# (b) %-28s %4d launches, avg %9.2f us, %d B/sample -> %7.1f GB/s" % (key, calls, us, b, samples * b / us / 1e3))
            else:
                say("# (b) %-28s not measured (not in the trace)" % key)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--skip-trace", action="store_true", help="leave (b) out")
    ap.add_argument("--probe", action="store_true", help="(internal) the child that runs under the kernel trace")
    args = ap.parse_args()
    if args.probe:
        return probe(args.rows, args.seconds)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import torch
    from speechseparation_amd import _native, mining
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    rows = args.rows
    model = BSRNN().eval().to("cuda:0")            # (untrained weights: the timing does not depend on them)
    mix, n = buffers(rows, args.seconds)
    H = n // HOP
    say("# %s, %s; %d rows x %d s at %d Hz = %d hops per row" % (torch.cuda.get_device_name(0), torch.version.hip, rows, args.seconds, RATE, H))
    clips = [mix[r] for r in range(rows)]
    est = torch.stack(model.separate_many_long(clips))
    out = torch.empty((rows, H, 2), device="cuda", dtype=torch.float64)
    ctx = model._context(mix.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        assert _native.lib.bsrnn_hop_activity(ctx, ctypes.c_void_p(mix.data_ptr()), n, ctypes.c_void_p(est.data_ptr()), H * HOP, None, rows, H,
                                              ctypes.c_void_p(out.data_ptr()), stream) == 0
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    say("# activity: %d hops, %d finite ratios, median 10 ln(ratio) %.2f" % (a[..., 0].size, int(np.isfinite(a[..., 0]).sum()),
                                                                              float(np.median(10 * np.log(a[..., 0][a[..., 0] > 0])))))
    us = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            call()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    med, gb = float(np.median(us)), rows * H * HOP * 8 / 1e9
    say("# (a) bsrnn_hop_activity, %d windows of %d calls between events: %.2f us per call [%.2f .. %.2f], %.3f GB read -> %.1f GB/s"
        % (REPEATS, CALLS, med, min(us), max(us), gb, gb / (med * 1e-6)))

    jobs = {"mine": lambda: mining.mine(model, clips), "separate_many_long": lambda: model.separate_many_long(clips)}
    t = {k: [] for k in jobs}
    for k, f in jobs.items():
        f()
    for _ in range(E2E_REPEATS):
        for k, f in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    for k in jobs:
        say("# (c) %-20s %9.2f ms per call [%.2f .. %.2f] of %d" % (k, float(np.median(t[k])), min(t[k]), max(t[k]), E2E_REPEATS))
    say("# (c) mine - separate_many_long = %.2f ms (activity launch, download of %d x %d x 2 doubles, the scanner on the host)"
        % (float(np.median(t["mine"])) - float(np.median(t["separate_many_long"])), rows, H))
    if not args.skip_trace:                        # last, in a process of its own: whatever becomes of it, the figures above stand
        torch.cuda.synchronize()
        traced(min(rows, TRACE_ROWS), args.seconds, say)


if __name__ == "__main__":
    main()
