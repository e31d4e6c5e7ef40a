#!/usr/bin/env python3
"""The ragged long-form evaluate, measured in one run on one GPU at the size a user validates at: 64 clips of one row each, unequal
lengths from 60 s down to 6 s at 44.1 kHz, longest first, 256 frames per segment.

  (a) `BSRNN.evaluate_long_ragged` beside `BSRNN.separate_long_ragged` alone on the same batch (already on the device, the estimate
      into a preallocated buffer), alternating: a host clock around calls that end in a device synchronise, after a warm-up of both.
      The difference is the metric side: per segment one more analysis (the clean signal's) and two reductions, once per call the
      INPUT_SDR launch, a memset and the download.  `workspace_rows()` of a model that has made only these calls, against the frame
      rows of the plan and of the rectangle.
  (b) what the mixture's analysis costs in the same call - the STFT stage of `separate_long_ragged` bracketed by events (a run of its
      own, after the timings) - as the yardstick for the clean signal's.
  (c) `BSRNN.evaluate_ragged` beside `evaluate_long_ragged` on a batch both forms can hold - every fourth clip, 16 rows - each on a
      model of its own, so `workspace_rows()` is that form's; and how far the two forms' numbers and estimates are apart.
  (d) the kernels of the metric side by kernel time: a child process of this tool under `rocprofv3 --kernel-trace --stats` makes the
      call of (a) three times.  The analysis kernel's figure covers the mixture's and the clean signal's launches alike.  It runs last
      and nothing else depends on it.

    python tools/evaluate_long_bench.py [--out profiles/evaluate_long_bench.txt] [--skip-trace] [--rows 64 --seconds 60 --segment-frames 256]
"""
import argparse
import csv
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
REPEATS = 5
TRACE_TIMEOUT_S = 300


def batch(rows, seconds):
    """mix, speech [rows, n_max] on the device and the rows' lengths, longest first: from `seconds` down to a tenth of it."""
    import torch
    n_max = RATE * seconds
    lens = [int(n_max * (1.0 - 0.9 * r / max(rows - 1, 1))) for r in range(rows)]
    g = torch.Generator(device="cuda").manual_seed(1)
    speech = 0.07 * torch.randn((rows, n_max), device="cuda", generator=g)
    mix = speech + 0.05 * torch.randn((rows, n_max), device="cuda", generator=g)
    return mix, speech, lens


def timed(jobs, repeats=REPEATS):
    """Every job once as a warm-up, then `repeats` rounds of all of them in turn; ms per call."""
    import torch
    t = {k: [] for k in jobs}
    for f in jobs.values():
        f()
    for _ in range(repeats):
        for k, f in jobs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return t


def probe(rows, seconds, seg):
    """The traced child: the call three times on the batch of (a)."""
    import torch
    from speechseparation_amd.bsrnn import BSRNN
    model = BSRNN().eval().to("cuda:0")
    mix, speech, lens = batch(rows, seconds)
    for _ in range(3):
        model.evaluate_long_ragged(mix, speech, lens, None, seg)
    torch.cuda.synchronize()


def traced(rows, seconds, seg, say):
    d = tempfile.mkdtemp(prefix="evaluate_long_bench_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--probe", "--rows", str(rows), "--seconds", str(seconds), "--segment-frames", str(seg)]
        proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
        try:
            stdout, _ = proc.communicate(timeout=TRACE_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            os.killpg(proc.pid, signal.SIGKILL)            # the profiler and the process under it
            proc.wait()
            say("# (d) kernel trace: not measured (the traced process did not end within %d s)" % TRACE_TIMEOUT_S)
            sys.exit(124)
        files = glob.glob(os.path.join(d, "*", "*kernel_stats.csv"))
        if proc.returncode != 0 or not files:
            say("# (d) kernel trace: not measured (rocprofv3 exit %d)" % proc.returncode)
            for ln in stdout.splitlines()[-5:]:
                say("#     " + ln)
            return
        say("# (d) kernel times from the trace of a child process (the batch of (a), three calls):")
        keys = ("stft_ragged_segment_kernel", "metric_time_ragged_segment_kernel", "metric_freq_ragged_segment_kernel",
                "metric_input_sdr_ragged_kernel")
        found = {}
        for r in csv.DictReader(open(files[0])):
            for key in keys:
                if key in r["Name"] and "istft" not in r["Name"]:
                    found[key] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
        for key in keys:
            if key in found:
                say("# (d) %-36s %4d launches, avg %8.2f us" % (key, found[key][0], found[key][1]))
            else:
                say("# (d) %-36s not measured (not in the trace)" % key)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trace", action="store_true", help="leave (d) out")
    ap.add_argument("--probe", action="store_true", help="(internal) the child that runs under the kernel trace")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--segment-frames", type=int, default=256)
    args = ap.parse_args()
    if args.probe:
        return probe(args.rows, args.seconds, args.segment_frames)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import torch
    from speechseparation_amd import _native, spec
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    rows, seg = args.rows, args.segment_frames
    mix, speech, lens = batch(rows, args.seconds)
    frames = [spec.n_frames(n) for n in lens]
    prefix, plan_rows = spec.long_plan(frames, seg)
    say("# tools/evaluate_long_bench.py, the shipped library")
    say("# %s, %s; %d clips of one row, %.1f .. %.1f s at %d Hz, longest first; %d frames per segment: %d segments, %d frame rows "
        "(real %d, rectangle %d)" % (torch.cuda.get_device_name(0), torch.version.hip, rows, lens[-1] / RATE, lens[0] / RATE, RATE, seg,
                                     len(prefix), plan_rows, sum(frames), rows * max(frames)))

    # (a) untrained weights: the timing does not depend on them
    model = BSRNN().eval().to("cuda:0")
    est = torch.empty((rows, (max(lens) // HOP) * HOP), device="cuda", dtype=torch.float32)
    jobs = {"evaluate_long_ragged": lambda: model.evaluate_long_ragged(mix, speech, lens, None, seg),
            "separate_long_ragged": lambda: model.separate_long_ragged(mix, lens, seg, out=est)}
    t = timed(jobs)
    med = {k: float(np.median(v)) for k, v in t.items()}
    for k in jobs:
        say("# (a) %-22s %9.2f ms per call [%.2f .. %.2f] of %d" % (k, med[k], min(t[k]), max(t[k]), REPEATS))
    diff = med["evaluate_long_ragged"] - med["separate_long_ragged"]
    say("# (a) evaluate - separate = %.2f ms = %.1f %% of the separation, %.3f ms per segment (the clean signal's analysis, two reductions; "
        "per call the INPUT_SDR launch, a memset, the download)" % (diff, 100.0 * diff / med["separate_long_ragged"], diff / len(prefix)))
    say("# (a) workspace_rows() = %d (rows x segment = %d; the rectangle would need %d)" % (model.workspace_rows(), rows * seg, rows * max(frames)))
    m = model.evaluate_long_ragged(mix, speech, lens, None, seg)
    say("# (a) clip 0: sdr %.4f dB, sisdr %.4f dB, loss %.6f; clip %d: sdr %.4f dB" % (m[0]["sdr"], m[0]["sisdr"], m[0]["loss"], rows - 1, m[-1]["sdr"]))

    # (b) the mixture's analysis inside the same call, by events (profiling slows the host: a run of its own)
    stft = [s for s in _native.stage_names() if "stft" in s.lower() and "istft" not in s.lower()]
    model.set_profiling(True)
    model.stage_times()
    model.separate_long_ragged(mix, lens, seg, out=est)
    torch.cuda.synchronize()
    st = model.stage_times()
    model.set_profiling(False)
    total = sum(v[0] for v in st.values())
    for s in stft:
        say("# (b) stage %-10s of separate_long_ragged: %.3f ms in %d launches (%.3f ms per segment) of %.2f ms in all bracketed stages; "
            "evaluate - separate is %.2f x that" % (s, st[s][0], st[s][1], st[s][0] / max(st[s][1], 1), total, diff / st[s][0] if st[s][0] else float("nan")))

    # (c) a batch both forms can hold, each form on a model of its own
    pick = list(range(0, rows, 4))
    sm, ss, sl = mix[pick].contiguous(), speech[pick].contiguous(), [lens[r] for r in pick]
    sf = [spec.n_frames(n) for n in sl]
    long_model, rag_model = BSRNN().eval(), BSRNN().eval()
    rag_model.load_state_dict(long_model.state_dict())          # (untrained, but the same weights: their numbers are compared below)
    long_model, rag_model = long_model.to("cuda:0"), rag_model.to("cuda:0")
    jobs = {"evaluate_long_ragged": lambda: long_model.evaluate_long_ragged(sm, ss, sl, None, seg),
            "evaluate_ragged": lambda: rag_model.evaluate_ragged(sm, ss, sl)}
    t = timed(jobs)
    say("# (c) %d of the clips (every fourth): %d frame rows in segments, %d in the rectangle" % (len(pick), spec.long_plan(sf, seg)[1], len(pick) * max(sf)))
    for k, mdl in (("evaluate_long_ragged", long_model), ("evaluate_ragged", rag_model)):
        say("# (c) %-22s %9.2f ms per call [%.2f .. %.2f] of %d, workspace_rows() = %d" % (
            k, float(np.median(t[k])), min(t[k]), max(t[k]), REPEATS, mdl.workspace_rows()))
    a = long_model.evaluate_long_ragged(sm, ss, sl, None, seg, return_estimate=True)
    b = rag_model.evaluate_ragged(sm, ss, sl, return_estimate=True)
    say("# (c) the two forms over the %d clips: largest |estimate difference| %.2e at |estimate|max %.2e; largest |difference| per figure:"
        % (len(pick), max(float((x["x_time"] - y["x_time"]).abs().max()) for x, y in zip(a, b)), max(float(y["x_time"].abs().max()) for y in b)))
    for k in ("sdr", "input_sdr", "sisdr", "separation_db"):
        say("# (c)   %-13s %.2e dB (values %.4f .. %.4f)" % (k, max(abs(x[k] - y[k]) for x, y in zip(a, b)), min(y[k] for y in b), max(y[k] for y in b)))
    for k in ("loss", "l1_time", "l1_re", "l1_im"):
        say("# (c)   %-13s %.2e relative" % (k, max(abs(x[k] - y[k]) / abs(y[k]) for x, y in zip(a, b))))
    del a, b
    if not args.skip_trace:                        # last, in a process of its own: whatever becomes of it, the figures above stand
        torch.cuda.synchronize()
        traced(rows, args.seconds, seg, say)


if __name__ == "__main__":
    main()
