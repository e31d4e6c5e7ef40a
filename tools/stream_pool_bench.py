#!/usr/bin/env python3
"""Session slots against their alternatives, on one GPU, inputs resident, deferred range policy, one hop per step.

Part 1, for S = 1, 8 and 32 live sessions of 2 rows each (REPORTED, no ratio is asked of it):
  (a) one bsrnn_stream_process_rows on ONE stream of 64 rows (32 slots): the S sessions' rows active with a wet / dry value per row,
      the other rows held - the row-masked kernels
  (b) S separate two-row streams, bsrnn_stream_step on each in turn (a context takes one call at a time)
  (p) StreamPool.step for the same S sessions: (a) plus the Python side's packing and unpacking of the sessions' tensors

Part 2, at C = 64 (a CHECK: the rows entry point with nothing held must cost what the plain call costs):
  (r) bsrnn_stream_process_rows, active = ones, mix_rows_dev = NULL      (f) the same with mix_rows_dev = ones: the row-masked kernels
  (q) bsrnn_stream_process
Every run of part 2 is a process of its own, and runs alternate between this build and, with --baseline-lib, another build of the
library (the parent commit's, which has no rows call: q only), twice each: the difference between the two runs of the SAME library
is the file's own run-to-run spread, and q of this build against q of the baseline is to be read against it.

Each figure is the median over REPEATS windows of a host clock around enough jobs to fill ~0.2 s, ending in a device synchronise; the
variants alternate inside every repeat, and min .. max of the windows is printed beside the median.

    python tools/stream_pool_bench.py [--baseline-lib PATH] [--out profiles/stream_rows_ab.txt]

--hops times the hop count per row (bsrnn_stream_process_hops) instead of part 1, the same way (several hops per call here):
  H1, the use case: the 64-row stream, 32 sessions of 2 rows whose counts are drawn from {1, 2, 3} (fixed seed).  (h) ONE process_hops
      call per tick against (g) what a build without it needs for the same audio: one process_rows per distinct count, the sessions of
      that count active.
  H2, the cost of the ragged form: (h) process_hops with every row at 7 of 8 hops - mixed counts, so nothing delegates - against
      (q) bsrnn_stream_process at 8 hops, C = 64, same process, alternating.
  H3, the plain calls: part 2 above, this build against --baseline-lib.

    python tools/stream_pool_bench.py --hops [--baseline-lib PATH] [--out profiles/stream_hops_ab.txt]

--rates times sessions at their own sample rates: the 64-row stream, 32 sessions of 2 rows whose rates are drawn from {16 000, 32 000,
48 000, 96 000} (fixed seed), each giving one hop's worth of audio at its rate per tick.  (a) StreamPool.feed of a pool with rates:
one inbound and one outbound resampler-bank call around the one process_hops; (b) the same tick from a pool without rates and one
Resampler per session and direction around one feed; (c) the two bank calls alone, through the C ABI.

    python tools/stream_pool_bench.py --rates [--out profiles/stream_rates_ab.txt]

--native times the pool as an object of the library (bsrnn_pool_*): the setting of H1 - the 64-row stream, 32 sessions of 2 rows whose
counts are drawn from {1, 2, 3} (fixed seed), every session giving whole hops per tick - four ways in one process, alternating:
  (a) StreamPool.feed            (b) NativeStreamPool.feed            (c) bsrnn_pool_feed through ctypes with prebuilt arrays
  (f) the bare bsrnn_stream_process_hops of the same counts: the floor; c - f is the price of the two copy launches and the table.
Then the plain calls, each run a process of its own, this build against --baseline-lib, twice each: part 2 above and, beside it, the
bsrnn_stream_process_hops of (f).

    python tools/stream_pool_bench.py --native [--baseline-lib PATH] [--out profiles/stream_pool_native_ab.txt]

--native-rates times the native pool's sessions at their own sample rates in the setting of --rates (the 64-row stream, 32 sessions of 2
rows, rates drawn from {16 000, 32 000, 48 000, 96 000}, one hop's worth of audio per session per tick), three ways in one process,
alternating:
  (a) StreamPool(rates=...).feed            (b) NativeRatePool.feed            (c) bsrnn_pool_feed through ctypes with prebuilt arrays
Two figures per arm: the wall time per tick (the windows above) and the stream time of one tick - two events around a single tick that
starts on an idle device, so the launch gaps of a host-bound tick are part of it.

    python tools/stream_pool_bench.py --native-rates [--out profiles/stream_pool_native_rates_ab.txt]
"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SESSIONS = (1, 8, 32)
ROWS = 2
SLOTS = 32
REPEATS = 7
WINDOW_S = 0.2
HOP = 1024
PLAIN_SHAPES = ((64, 1), (64, 8))
RATES = (16000, 32000, 48000, 96000)
MODEL_RATE = 44100


def measure(jobs, sync):
    """{name: job} -> {name: (median, min, max)} in us per job; the jobs alternate inside every repeat."""
    import numpy as np
    n = {}
    for k, f in jobs.items():                     # warm-up, and how many jobs fill a window
        for _ in range(3):
            f()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            f()
        sync()
        n[k] = max(3, int(WINDOW_S / max((time.perf_counter() - t0) / 3, 1e-6)))
    t = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, f in jobs.items():
            sync()
            t0 = time.perf_counter()
            for _ in range(n[k]):
                f()
            sync()
            t[k].append((time.perf_counter() - t0) / n[k] * 1e6)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def stream_time(jobs, sync, repeats=25):
    """{name: job} -> {name: (median, min, max)} in us: two events around ONE job that starts on an idle device, alternating."""
    import numpy as np
    import torch
    t = {k: [] for k in jobs}
    for _ in range(repeats):
        for k, f in jobs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            e0.record()
            f()
            e1.record()
            sync()
            t[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def cell(v):
    return "%9.1f [%8.1f .. %8.1f]" % v


def setup():
    import torch
    from speechseparation_amd import weights
    from speechseparation_amd.bsrnn import BSRNN
    assert torch.cuda.is_available(), "needs a GPU"
    sd = weights.synth_state_dict(None, seed=0)
    model = BSRNN().eval()
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model = model.to("cuda:0")
    model.set_range_policy("deferred")
    return model


def tick_counts():
    """The hop counts of one tick of H1 / --native: per session, and per row of the 64-row stream."""
    import random
    rnd = random.Random(7)
    per_session = [rnd.choice((1, 2, 3)) for _ in range(SLOTS)]
    return per_session, [per_session[r // ROWS] for r in range(SLOTS * ROWS)]


def plain_only():
    """Part 2 in this process, on the library BSRNN_HIP_LIB names (default: the in-tree build), through the C ABI alone - the same
    harness for a build with and without the rows calls: one line per shape."""
    import numpy as np
    from speechseparation_amd import spec, weights
    path = os.environ.get("BSRNN_HIP_LIB") or os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
    lib = ctypes.CDLL(path)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sig = {"bsrnn_create": [ctypes.c_int, ctypes.POINTER(i32), i32, ctypes.POINTER(vp)], "bsrnn_set_param": [vp, ctypes.c_char_p, vp, i64],
           "bsrnn_commit_params": [vp], "bsrnn_set_range_policy": [vp, i32], "bsrnn_stream_create": [vp, i32, ctypes.POINTER(vp)],
           "bsrnn_stream_reserve": [vp, i32], "bsrnn_stream_process": [vp, vp, vp, i32, ctypes.c_float, vp], "bsrnn_dev_alloc": [vp, i64, ctypes.POINTER(vp)],
           "bsrnn_copy_h2d": [vp, vp, vp, i64], "bsrnn_sync": [vp, vp], "bsrnn_stream_destroy": [vp], "bsrnn_dev_free": [vp, vp]}
    has_rows = hasattr(lib, "bsrnn_stream_process_rows")
    if has_rows:
        sig["bsrnn_stream_process_rows"] = [vp, vp, vp, i32, vp, vp, ctypes.c_float, vp]
    for name, args in sig.items():
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = None if name == "bsrnn_stream_destroy" else ctypes.c_int
    lib.bsrnn_last_error.restype = ctypes.c_char_p

    def check(rc):
        if rc != 0:
            raise SystemExit("libbsrnn_hip: error %d: %s" % (rc, lib.bsrnn_last_error().decode()))
    v = spec.generate_bandsplits()[0]
    ctx = vp()
    check(lib.bsrnn_create(0, (i32 * len(v))(*v), len(v), ctypes.byref(ctx)))
    for key, val in weights.synth_state_dict(None, seed=0).items():
        a = np.ascontiguousarray(val, np.float32)
        check(lib.bsrnn_set_param(ctx, key.encode(), a.ctypes.data_as(vp), a.size))
    check(lib.bsrnn_commit_params(ctx))
    check(lib.bsrnn_set_range_policy(ctx, 0))                # deferred

    def on_device(a):
        p = vp()
        check(lib.bsrnn_dev_alloc(ctx, a.nbytes, ctypes.byref(p)))
        check(lib.bsrnn_copy_h2d(ctx, p, a.ctypes.data_as(vp), a.nbytes))
        return p
    one = ctypes.c_float(1.0)
    for C, L in PLAIN_SHAPES:
        st = vp()
        check(lib.bsrnn_stream_create(ctx, C, ctypes.byref(st)))
        check(lib.bsrnn_stream_reserve(st, L))
        wave = on_device(np.ascontiguousarray(weights.synth_waveform(C, L * HOP, seed=5), np.float32))
        out = on_device(np.zeros((C, L * HOP), np.float32))
        jobs = {"q": lambda: check(lib.bsrnn_stream_process(st, wave, out, L, one, None))}
        if has_rows:
            ones = (ctypes.c_uint8 * C)(*([1] * C))
            mix_rows = on_device(np.ones(C, np.float32))
            jobs["r"] = lambda: check(lib.bsrnn_stream_process_rows(st, wave, out, L, ones, None, one, None))
            jobs["f"] = lambda: check(lib.bsrnn_stream_process_rows(st, wave, out, L, ones, mix_rows, one, None))
        res = measure(jobs, lambda: check(lib.bsrnn_sync(ctx, None)))
        print("PLAIN %d %d %s" % (C, L, " ".join("%s %.2f %.2f %.2f" % ((k,) + v) for k, v in res.items())), flush=True)
        lib.bsrnn_stream_destroy(st)
    if hasattr(lib, "bsrnn_stream_process_hops"):              # the hops call of one tick of H1 / --native
        lib.bsrnn_stream_process_hops.argtypes = [vp, vp, vp, i32, vp, vp, ctypes.c_float, vp]
        lib.bsrnn_stream_process_hops.restype = ctypes.c_int
        counts = tick_counts()[1]
        C, L = len(counts), max(counts)
        st = vp()
        check(lib.bsrnn_stream_create(ctx, C, ctypes.byref(st)))
        check(lib.bsrnn_stream_reserve(st, L))
        wave = on_device(np.ascontiguousarray(weights.synth_waveform(C, L * HOP, seed=5), np.float32))
        out = on_device(np.zeros((C, L * HOP), np.float32))
        cnt = (i32 * C)(*counts)
        res = measure({"h": lambda: check(lib.bsrnn_stream_process_hops(st, wave, out, L, cnt, None, one, None))}, lambda: check(lib.bsrnn_sync(ctx, None)))
        print("HOPS %d %d %.2f %.2f %.2f" % ((C, L) + res["h"]), flush=True)
        lib.bsrnn_stream_destroy(st)


def plain_runs(baseline_lib):
    """Part 2: child processes, before this one opens the GPU -> [(library, C, L, {variant: (median, min, max)})]."""
    runs = [("this build", None), ("this build", None)]
    if baseline_lib:
        base = os.path.abspath(baseline_lib)
        assert os.path.exists(base), base
        runs = [("baseline", base), ("this build", None), ("baseline", base), ("this build", None)]
    part2 = []
    HOPS_RUNS[:] = []
    for name, path in runs:
        env = dict(os.environ)
        env.pop("BSRNN_HIP_LIB", None)
        if path:
            env["BSRNN_HIP_LIB"] = path
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-only"], env=env, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            raise SystemExit("part 2 run on %s failed with status %d" % (name, out.returncode))
        for ln in out.stdout.splitlines():
            if ln.startswith("PLAIN "):
                f = ln.split()
                vals = {f[i]: tuple(float(x) for x in f[i + 1:i + 4]) for i in range(3, len(f), 4)}
                part2.append((name, int(f[1]), int(f[2]), vals))
            elif ln.startswith("HOPS "):
                f = ln.split()
                HOPS_RUNS.append((name, int(f[1]), int(f[2]), tuple(float(x) for x in f[3:6])))
    return part2


HOPS_RUNS = []          # plain_runs: [(library, C, L, (median, min, max))] of the bare hops call, one per child process


def report_hops_runs(say):
    say("# bsrnn_stream_process_hops, C = 64, counts from {1, 2, 3} (the tick of --native), each line a process of its own")
    say("%-11s %4s %4s %28s" % ("library", "C", "L", "h us"))
    for name, Cc, L, v in HOPS_RUNS:
        say("%-11s %4d %4d %28s" % (name, Cc, L, cell(v)))
    h = {n: [v[0] for (nm, _, _, v) in HOPS_RUNS if nm == n] for n in ("baseline", "this build")}
    two = [v for v in h.values() if len(v) == 2]
    if two:
        line = "run-to-run spread of h (same library, two processes) %.1f us" % max(abs(v[0] - v[1]) for v in two)
        if len(h["baseline"]) == 2 and len(h["this build"]) == 2:
            line += "; h this build - h baseline (means of the two runs) %+.1f us" % (sum(h["this build"]) / 2 - sum(h["baseline"]) / 2)
        say(line)


def report_plain(say, part2):
    say("# part 2: C = 64, nothing held, each line a process of its own.  q = stream_process, r = stream_process_rows(active = ones, "
        "mix_rows = NULL), f = the same with mix_rows = ones (row-masked kernels)")
    say("%-11s %4s %4s %28s %28s %28s" % ("library", "C", "L", "q us", "r us", "f us"))
    for name, Cc, L, vals in part2:
        say("%-11s %4d %4d %28s %28s %28s" % (name, Cc, L, cell(vals["q"]), cell(vals["r"]) if "r" in vals else "-", cell(vals["f"]) if "f" in vals else "-"))
    for Cc, L in PLAIN_SHAPES:
        q = {n: [v["q"][0] for (nm, c2, l2, v) in part2 if nm == n and (c2, l2) == (Cc, L)] for n in ("baseline", "this build")}
        spread = max(abs(v[0] - v[1]) for v in q.values() if len(v) == 2)
        line = "C %d L %d: run-to-run spread of q (same library, two processes) %.1f us" % (Cc, L, spread)
        if q["baseline"]:
            line += "; q this build - q baseline (means of the two runs) %+.1f us" % (sum(q["this build"]) / 2 - sum(q["baseline"]) / 2)
        rr = [v["r"][0] - v["q"][0] for (nm, c2, l2, v) in part2 if nm == "this build" and (c2, l2) == (Cc, L)]
        line += "; r - q inside a run %s us" % ", ".join("%+.1f" % x for x in rr)
        say(line)


def hops_parts(say):
    """H1 and H2 of --hops, in this process."""
    import torch
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    lib, check = _native.lib, _native.check
    model = setup()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    one = ctypes.c_float(1.0)
    C = SLOTS * ROWS
    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# us per call (or per tick): median [min .. max] of %d windows of ~%.1f s; inputs resident, deferred range policy" % (REPEATS, WINDOW_S))
    wide = StreamingSeparator(model, channels=C, device="cuda:0")
    wide.reserve(8)
    per_session, counts = tick_counts()
    L = max(counts)
    waves = {k: torch.from_numpy(weights.synth_waveform(C, k * HOP, seed=5)).cuda() for k in (1, 2, 3, 8)}
    outs = {k: torch.empty_like(w) for k, w in waves.items()}
    cnt = (ctypes.c_int32 * C)(*counts)
    flags = {k: (ctypes.c_uint8 * C)(*[int(c == k) for c in counts]) for k in sorted(set(counts))}

    def job_h():
        check(lib.bsrnn_stream_process_hops(wide._h, ptr(waves[L]), ptr(outs[L]), L, cnt, None, one, None))

    def job_g():
        for k, fl in flags.items():
            check(lib.bsrnn_stream_process_rows(wide._h, ptr(waves[k]), ptr(outs[k]), k, fl, None, one, None))

    r = measure({"h": job_h, "g": job_g}, torch.cuda.synchronize)
    model.sync()
    say("# H1: %d-row stream, %d sessions of %d rows, counts from {1, 2, 3} (seed 7: %s sessions at 1 / 2 / 3 hops); per tick" % (
        C, SLOTS, ROWS, " / ".join(str(per_session.count(k)) for k in (1, 2, 3))))
    say("%-44s %28s" % ("h  one process_hops (L = %d)" % L, cell(r["h"])))
    say("%-44s %28s" % ("g  one process_rows per distinct count (%d)" % len(flags), cell(r["g"])))
    say("g / h = %.2f" % (r["g"][0] / r["h"][0]))
    say("")
    seven = (ctypes.c_int32 * C)(*([7] * C))

    def job_h8():
        check(lib.bsrnn_stream_process_hops(wide._h, ptr(waves[8]), ptr(outs[8]), 8, seven, None, one, None))

    def job_q8():
        check(lib.bsrnn_stream_process(wide._h, ptr(waves[8]), ptr(outs[8]), 8, one, None))

    r = measure({"h": job_h8, "q": job_q8}, torch.cuda.synchronize)
    model.sync()
    say("# H2: C = %d, L = 8.  h = process_hops with every row at 7 hops (the ragged kernels), q = stream_process at 8 hops" % C)
    say("%-44s %28s" % ("h  process_hops, all rows 7 of 8", cell(r["h"])))
    say("%-44s %28s" % ("q  stream_process, 8 hops", cell(r["q"])))
    say("h - q = %+.1f us (%.1f %%)" % (r["h"][0] - r["q"][0], 100.0 * (r["h"][0] / r["q"][0] - 1.0)))
    say("")


def rates_part(say):
    """--rates, in this process."""
    import random
    import torch
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import Resampler, ResamplerBank, StreamPool
    lib, check = _native.lib, _native.check
    model = setup()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    C = SLOTS * ROWS
    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# us per tick: median [min .. max] of %d windows of ~%.1f s; inputs resident, deferred range policy" % (REPEATS, WINDOW_S))
    rnd = random.Random(7)
    per_session = [rnd.choice(RATES) for _ in range(SLOTS)]
    n_of = {r: (HOP * r + MODEL_RATE // 2) // MODEL_RATE for r in RATES}           # one hop's worth of audio at rate r
    audio = torch.from_numpy(weights.synth_waveform(C, max(n_of.values()), seed=5)).cuda()
    blocks = [audio[ROWS * i:ROWS * (i + 1), :n_of[r]].contiguous() for i, r in enumerate(per_session)]
    # (a) the pool with its banks
    pool = StreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0", rates=RATES)
    sids = [pool.open(sample_rate=r) for r in per_session]
    chunks = {sids[i]: blocks[i] for i in range(SLOTS)}
    # (b) a pool without rates and one Resampler per session and direction
    plain = StreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0")
    psids = [plain.open() for _ in range(SLOTS)]
    rin = [Resampler(model, ROWS, r, MODEL_RATE) for r in per_session]
    rout = [Resampler(model, ROWS, MODEL_RATE, r) for r in per_session]
    # (c) the two bank calls alone, through the C ABI: the tick's counts inbound, one hop per row outbound
    bank_in = ResamplerBank(model, C, [(r, MODEL_RATE) for r in RATES])
    bank_out = ResamplerBank(model, C, [(MODEL_RATE, r) for r in RATES])
    for i, r in enumerate(per_session):
        bank_in.assign(list(range(ROWS * i, ROWS * (i + 1))), RATES.index(r))
        bank_out.assign(list(range(ROWS * i, ROWS * (i + 1))), RATES.index(r))
    wave_in = torch.zeros((C, max(n_of.values())), device="cuda")
    for i, b in enumerate(blocks):
        wave_in[ROWS * i:ROWS * (i + 1), :b.shape[1]] = b
    i64 = ctypes.c_int64
    counts_in = (i64 * C)(*[n_of[per_session[r // ROWS]] for r in range(C)])
    counts_hop = (i64 * C)(*([HOP] * C))
    n_out = (i64 * C)()
    conv = torch.empty((C, HOP + 64), device="cuda")
    wave_hop = torch.from_numpy(weights.synth_waveform(C, HOP, seed=6)).cuda()
    back = torch.empty((C, 4 * HOP), device="cuda")

    def job_a():
        pool.feed(chunks)

    def job_b():
        res = plain.feed({psids[i]: rin[i].process(blocks[i]) for i in range(SLOTS)})
        for i in range(SLOTS):
            o = res[psids[i]]
            if o.shape[1]:
                rout[i].process(o)

    def job_c():
        check(lib.bsrnn_resampler_bank_process(bank_in._h, ptr(wave_in), wave_in.stride(0), counts_in, ptr(conv), conv.stride(0), n_out, None))
        check(lib.bsrnn_resampler_bank_process(bank_out._h, ptr(wave_hop), HOP, counts_hop, ptr(back), back.stride(0), n_out, None))

    r = measure({"a": job_a, "b": job_b, "c": job_c}, torch.cuda.synchronize)
    model.sync()
    say("# %d-row stream, %d sessions of %d rows, rates from {%s} (seed 7: %s sessions), one hop's worth of audio per session per tick" % (
        C, SLOTS, ROWS, ", ".join(str(x) for x in RATES), " / ".join(str(per_session.count(x)) for x in RATES)))
    say("%-64s %28s" % ("a  StreamPool.feed with the two resampler banks", cell(r["a"])))
    say("%-64s %28s" % ("b  one Resampler per session and direction around one feed", cell(r["b"])))
    say("%-64s %28s" % ("c  the two bank calls alone (C ABI)", cell(r["c"])))
    say("b / a = %.2f; a - c = %.1f us" % (r["b"][0] / r["a"][0], r["a"][0] - r["c"][0]))
    say("")


def native_rates_part(say):
    """--native-rates, in this process."""
    import random
    import torch
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import NativeRatePool, StreamPool
    lib, check = _native.lib, _native.check
    model = setup()
    one = ctypes.c_float(1.0)
    C = SLOTS * ROWS
    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# us per tick: median [min .. max]; wall: %d windows of ~%.1f s; stream: 25 single ticks between two events; inputs resident, "
        "deferred range policy" % (REPEATS, WINDOW_S))
    rnd = random.Random(7)
    per_session = [rnd.choice(RATES) for _ in range(SLOTS)]
    n_of = {r: (HOP * r + MODEL_RATE // 2) // MODEL_RATE for r in RATES}           # one hop's worth of audio at rate r
    audio = torch.from_numpy(weights.synth_waveform(C, max(n_of.values()), seed=5)).cuda()
    blocks = [audio[ROWS * i:ROWS * (i + 1), :n_of[r]].contiguous() for i, r in enumerate(per_session)]
    # (a) the Python pool with its banks
    pool = StreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0", rates=RATES)
    sids = [pool.open(sample_rate=r) for r in per_session]
    chunks = {sids[i]: blocks[i] for i in range(SLOTS)}
    # (b) the native pool through its Python class
    npool = NativeRatePool(model, SLOTS, rows_per_session=ROWS, device="cuda:0", max_hops=8, rates=RATES, max_block=max(n_of.values()))
    nsids = [npool.open(sample_rate=r) for r in per_session]
    nchunks = {nsids[i]: blocks[i] for i in range(SLOTS)}
    # (c) the library call alone, every array built once; a tick gives one hop's worth or two, so three fit every output row
    cpool = NativeRatePool(model, SLOTS, rows_per_session=ROWS, device="cuda:0", max_hops=8, rates=RATES, max_block=max(n_of.values()))
    for r in per_session:
        cpool.open(sample_rate=r)
    h_pool = cpool._pool()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    outs = [torch.empty((ROWS, 3 * b.shape[1] + 64), device="cuda") for b in blocks]
    a_slots = (i32 * SLOTS)(*range(SLOTS))
    a_in = (vp * SLOTS)(*[b.data_ptr() for b in blocks])
    a_out = (vp * SLOTS)(*[o.data_ptr() for o in outs])
    a_n = (i64 * SLOTS)(*[b.shape[1] for b in blocks])
    a_os = (i64 * SLOTS)(*[o.shape[1] for o in outs])
    a_got = (i64 * SLOTS)()

    def job_a():
        pool.feed(chunks)

    def job_b():
        npool.feed(nchunks)

    def job_c():
        check(lib.bsrnn_pool_feed(h_pool, SLOTS, a_slots, a_in, a_n, a_n, a_out, a_os, a_got, None, one, None))

    jobs = {"a": job_a, "b": job_b, "c": job_c}
    r = measure(jobs, torch.cuda.synchronize)
    g = stream_time(jobs, torch.cuda.synchronize)
    model.sync()
    say("# %d-row stream, %d sessions of %d rows, rates from {%s} (seed 7: %s sessions), one hop's worth of audio per session per tick" % (
        C, SLOTS, ROWS, ", ".join(str(x) for x in RATES), " / ".join(str(per_session.count(x)) for x in RATES)))
    say("%-56s %28s %28s" % ("", "wall", "stream"))
    say("%-56s %28s %28s" % ("a  StreamPool(rates=...).feed", cell(r["a"]), cell(g["a"])))
    say("%-56s %28s %28s" % ("b  NativeRatePool.feed", cell(r["b"]), cell(g["b"])))
    say("%-56s %28s %28s" % ("c  bsrnn_pool_feed through ctypes, prebuilt arrays", cell(r["c"]), cell(g["c"])))
    say("wall: a / b = %.2f, a / c = %.2f, b - c = %+.1f us (the Python around the call); b's windows lie wholly below a's: %s" % (
        r["a"][0] / r["b"][0], r["a"][0] / r["c"][0], r["b"][0] - r["c"][0], "yes" if r["b"][2] < r["a"][1] else "NO"))
    say("stream: a / b = %.2f, a / c = %.2f" % (g["a"][0] / g["b"][0], g["a"][0] / g["c"][0]))
    say("")


def native_part(say):
    """--native, in this process."""
    import torch
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import NativeStreamPool, StreamingSeparator, StreamPool
    lib, check = _native.lib, _native.check
    model = setup()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    one = ctypes.c_float(1.0)
    C = SLOTS * ROWS
    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# us per tick: median [min .. max] of %d windows of ~%.1f s; inputs resident, deferred range policy" % (REPEATS, WINDOW_S))
    per_session, counts = tick_counts()
    L = max(counts)
    audio = torch.from_numpy(weights.synth_waveform(C, L * HOP, seed=5)).cuda()
    blocks = [audio[ROWS * i:ROWS * (i + 1), :h * HOP].contiguous() for i, h in enumerate(per_session)]
    # (a) the Python pool
    pool = StreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0")
    sids = [pool.open() for _ in range(SLOTS)]
    chunks = {sids[i]: blocks[i] for i in range(SLOTS)}
    # (b) the native pool through its Python class
    npool = NativeStreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0", max_hops=8)
    nsids = [npool.open() for _ in range(SLOTS)]
    nchunks = {nsids[i]: blocks[i] for i in range(SLOTS)}
    # (c) the library call alone, every array built once
    cpool = NativeStreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0", max_hops=8)
    for _ in range(SLOTS):
        cpool.open()
    h_pool = cpool._pool()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    outs = [torch.empty_like(b) for b in blocks]
    a_slots = (i32 * SLOTS)(*range(SLOTS))
    a_in = (vp * SLOTS)(*[b.data_ptr() for b in blocks])
    a_out = (vp * SLOTS)(*[o.data_ptr() for o in outs])
    a_n = (i64 * SLOTS)(*[b.shape[1] for b in blocks])
    a_got = (i64 * SLOTS)()
    # (f) the floor: the bare hops call of the same counts
    wide = StreamingSeparator(model, channels=C, device="cuda:0")
    wide.reserve(8)
    wave = audio.contiguous()
    wout = torch.empty_like(wave)
    cnt = (i32 * C)(*counts)

    def job_a():
        pool.feed(chunks)

    def job_b():
        npool.feed(nchunks)

    def job_c():
        check(lib.bsrnn_pool_feed(h_pool, SLOTS, a_slots, a_in, a_n, a_n, a_out, a_n, a_got, None, one, None))

    def job_f():
        check(lib.bsrnn_stream_process_hops(wide._h, ptr(wave), ptr(wout), L, cnt, None, one, None))

    r = measure({"a": job_a, "b": job_b, "c": job_c, "f": job_f}, torch.cuda.synchronize)
    model.sync()
    assert list(a_got) == list(a_n)
    say("# %d-row stream, %d sessions of %d rows, counts from {1, 2, 3} (seed 7: %s sessions at 1 / 2 / 3 hops), whole hops per session per tick" % (
        C, SLOTS, ROWS, " / ".join(str(per_session.count(k)) for k in (1, 2, 3))))
    say("%-64s %28s" % ("a  StreamPool.feed", cell(r["a"])))
    say("%-64s %28s" % ("b  NativeStreamPool.feed", cell(r["b"])))
    say("%-64s %28s" % ("c  bsrnn_pool_feed through ctypes, prebuilt arrays", cell(r["c"])))
    say("%-64s %28s" % ("f  bsrnn_stream_process_hops alone (L = %d): the floor" % L, cell(r["f"])))
    say("b's windows lie wholly below a's: %s (largest b %.1f us, smallest a %.1f us); a / b = %.2f" % (
        "yes" if r["b"][2] < r["a"][1] else "NO", r["b"][2], r["a"][1], r["a"][0] / r["b"][0]))
    say("c - f = %+.1f us: the gather and scatter launches and the table of one tick; b - c = %+.1f us: the Python around the call" % (
        r["c"][0] - r["f"][0], r["b"][0] - r["c"][0]))
    say("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rates", action="store_true", help="time StreamPool.feed with sessions at their own sample rates instead")
    ap.add_argument("--baseline-lib", default=None, help="another build of libbsrnn_hip.so (the parent commit's) for part 2")
    ap.add_argument("--hops", action="store_true", help="time bsrnn_stream_process_hops (H1 - H3 above) instead of part 1")
    ap.add_argument("--native", action="store_true", help="time the native session pool (bsrnn_pool_feed, NativeStreamPool) instead of part 1")
    ap.add_argument("--native-rates", action="store_true", help="time the native pool's sessions at their own sample rates against StreamPool(rates=...)")
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.plain_only:
        return plain_only()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.native_rates:
        native_rates_part(say)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    if args.rates:
        rates_part(say)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    part2 = plain_runs(args.baseline_lib)
    if args.native:
        native_part(say)
        report_plain(say, part2)
        say("")
        report_hops_runs(say)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    if args.hops:
        hops_parts(say)
        say("# H3 = part 2:")
        report_plain(say, part2)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return

    import torch
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import StreamingSeparator, StreamPool
    lib, check = _native.lib, _native.check
    model = setup()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    one = ctypes.c_float(1.0)
    say("# %s, %s, compute mode %s" % (torch.cuda.get_device_name(0), torch.version.hip, _native.compute_mode()))
    say("# us per step of one hop: median [min .. max] of %d windows of ~%.1f s" % (REPEATS, WINDOW_S))
    say("# part 1: S sessions of %d rows.  a = one process_rows on a %d-row stream (S sessions active, per-row mix, the rest held), "
        "b = S two-row streams stepped in turn, p = StreamPool.step" % (ROWS, SLOTS * ROWS))
    say("%4s %28s %28s %28s %8s %8s" % ("S", "a us", "b us", "p us", "b/a", "b/p"))
    C = SLOTS * ROWS
    wide = StreamingSeparator(model, channels=C, device="cuda:0")
    pool = StreamPool(model, SLOTS, rows_per_session=ROWS, device="cuda:0")
    sids = [pool.open() for _ in range(SLOTS)]
    singles = [StreamingSeparator(model, channels=ROWS, device="cuda:0") for _ in range(max(SESSIONS))]
    wave = torch.from_numpy(weights.synth_waveform(C, HOP, seed=5)).cuda()
    out = torch.empty_like(wave)
    mix_rows = torch.ones(C, device="cuda")
    pairs = [wave[ROWS * i:ROWS * (i + 1)].contiguous() for i in range(SLOTS)]
    pair_out = torch.empty((ROWS, HOP), device="cuda")
    for S in SESSIONS:
        active = (ctypes.c_uint8 * C)(*([1] * (ROWS * S) + [0] * (C - ROWS * S)))
        chunks = {sids[i]: pairs[i] for i in range(S)}
        mixes = {sids[i]: 1.0 for i in range(S)}

        def job_a():
            check(lib.bsrnn_stream_process_rows(wide._h, ptr(wave), ptr(out), 1, active, ptr(mix_rows), one, None))

        def job_b():
            for i in range(S):
                check(lib.bsrnn_stream_step(singles[i]._h, ptr(pairs[i]), ptr(pair_out), one, None))

        def job_p():
            pool.step(chunks, mixes)

        r = measure({"a": job_a, "b": job_b, "p": job_p}, torch.cuda.synchronize)
        model.sync()
        say("%4d %28s %28s %28s %8.2f %8.2f" % (S, cell(r["a"]), cell(r["b"]), cell(r["p"]), r["b"][0] / r["a"][0], r["b"][0] / r["p"][0]))
    say("")
    report_plain(say, part2)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
