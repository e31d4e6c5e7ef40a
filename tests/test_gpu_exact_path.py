"""The exact-fp32 path at every call shape, the range guard's re-runs onto it, and aliased buffers.

Under the default range policy (include/bsrnn_hip.h) a call whose operands leave the fp16x2 range is run again on the exact-fp32
kernels before it returns, so these kernels carry "rc 0 always comes with correct numbers".  Here they run in a child process under
BSRNN_GEMM=f32 BSRNN_LSTM=f32 (the modes are read once per process) at the shapes where tilings go wrong (m-tiles and their tails,
the time-axis kernel's 8-step staging chunks and its partial groups of 4 sequences, GEMV calls of a few frame rows, row blocks, long
sequences), against the float64 oracle at the suite's rounding-level bound.  The re-runs of the default mode are then checked at the
shapes where the default flow differs most from the exact one (overlapped dual path, eight sequences per workgroup, two row blocks,
the small band block): the guard tripped (witness), the result is accurate, it equals the f32 child's bits (no fp16x2 launch survives
into the re-run), and nothing lasts.  Last, every entry point called with an output overlapping an input that the re-run reads either
refuses (BSRNN_EARG) or returns the numbers of the non-aliased call."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

BIG_X = 25000.0          # synth_tensor scale of out-of-range spectra: 100 x the scale=250 input of test_gpu_edges.py, |x| up to ~1e5
BIG_WAVE = 3e4           # waveforms far outside [-1, 1], as in test_gpu_edges.py
EARG = 1


def table(name):
    from speechseparation_amd import spec
    return spec.variant_bandsplits("41" if name == "41" else "default")


_SD = {}


def state_dict(name, w):
    """Weights per (table, set): 'default' as the suite's sd_default / 'hot' (lstm_gain = 3, saturating gates) as sd_hot."""
    from speechseparation_amd import weights
    key = (name, w)
    if key not in _SD:
        v = None if name == "12" else table(name)
        seed = (0 if w == "default" else 1) + (3 if name == "41" else 0)
        _SD[key] = weights.synth_state_dict(v, seed=seed, lstm_gain=3.0 if w == "hot" else 1.0)
    return _SD[key]


def case(name, kind, tab="12", w="default", rows=None, **kw):
    return dict(name=name, kind=kind, table=tab, w=w, rows=rows, **kw)


# Part 1: exact-fp32 child against the oracle.  `rows`: the rows the oracle checks (None = all); rows are independent.
CASES = [
    case("fwd 1x1", "forward", C=1, T=1),                       # GEMV path (M <= 4)
    case("fwd 1x4", "forward", w="hot", C=1, T=4),
    case("fwd 1x5", "forward", C=1, T=5),                       # first call past the GEMV edge
    case("fwd 3x3", "forward", w="hot", C=3, T=3),              # band tile tail (M % 16)
    case("fwd 2x7", "forward", C=2, T=7),                       # time kernel: around its 8-step staging chunk
    case("fwd 2x9", "forward", w="hot", C=2, T=9),
    case("fwd 1x17", "forward", C=1, T=17),
    case("fwd 2x64", "forward", w="hot", C=2, T=64),            # M = 128, T >= 32 layout
    case("fwd 3x43", "forward", C=3, T=43),                     # M = 129, T >= 32 layout without vec4
    case("fwd 17x131", "forward", w="hot", C=17, T=131, rows=[0, 1, 8, 16]),      # T > 128 layout tiles, 18 m-tiles
    case("fwd 64x126", "forward", C=64, T=126, rows=[0, 31, 32, 63]),            # the metric shape: 63 m-tiles, mchunk 2
    case("fwd41 1x9", "forward", tab="41", w="hot", C=1, T=9),  # 41 sequences: a partial last group of 4
    case("fwd41 3x40", "forward", tab="41", C=3, T=40),         # 123 sequences
    case("chunk 5x1", "chunk", w="hot", C=5, L=[1]),
    case("chunk 64x1", "chunk", C=64, L=[1]),
    case("chunk 3x20+3x13", "chunk", w="hot", C=3, L=[20, 13]),  # chained: the state of the first call feeds the second
    case("chunk41 3x17", "chunk", tab="41", C=3, L=[17]),
    case("dual 3x12", "dual", w="hot", C=3, T=12),
    case("dual 64x40", "dual", C=64, T=40, rows=[0, 31, 32, 63]),
    case("sep R1 n1025", "separate", R=1, n=1025),
    case("sep R130", "separate", w="hot", R=130, n=16 * 1024 + 9, rows=[0, 64, 65, 129]),   # two row blocks in the f32 mode
    case("sep R2 long", "separate", R=2, n=599 * 1024 + 5),    # T = 600
    case("stream C2x5", "stream", w="hot", C=2, steps=5),
    case("stream C64x2", "stream", C=64, steps=2),
]

# Part 2: the re-runs of the default mode; the child runs the same calls in the f32 mode for the bit comparison.
RERUN = [
    case("rerun overlapped 16x64", "forward", C=16, T=64, big=True, rows=[0, 7, 8, 15], overlapped=True),
    case("rerun 8 seqs 96x40", "forward", C=96, T=40, big=True, rows=[0, 47, 48, 95], overlapped=True),
    case("rerun row blocks R200", "separate", R=200, n=16 * 1024 + 9, big=True, rows=[0, 99, 100, 199]),
    case("rerun chunk 16x40", "chunk", C=16, L=[40], big=True, rows=[0, 15]),
    case("rerun dual 16x40", "dual", C=16, T=40, big=True, rows=[0, 15]),
    # (calls of <= 4 frame rows run their Linear layers as exact-fp32 GEMVs: only the LSTM operands can trip the guard, so the input is
    # scaled until the band-split output z, ~1.5e-2 |x|, leaves the fp16 range)
    case("rerun small 1x3", "forward", C=1, T=3, big=True, xscale=5e6),
    case("rerun small 2x4", "forward", C=2, T=4, big=True, xscale=5e6),
    case("rerun 41 bands 8x40", "forward", tab="41", C=8, T=40, big=True, rows=[0, 7]),
    case("rerun evaluate R130", "evaluate", R=130, n=6 * 1024 + 9, big=True, rows=[0, 129]),
]


def inputs(c, in_range=False):
    """The numpy inputs of a case, from seeds (in_range: the same shapes at audio scale, for the follow-up call of part 2)."""
    from speechseparation_amd import weights
    i = (CASES + RERUN).index(c)
    seed = 20000 + 100 * i + (50 if in_range else 0)
    big = c.get("big") and not in_range
    K = len(table(c["table"]))
    k = c["kind"]
    if k == "forward":
        return {"x": weights.synth_tensor((c["C"], 2050, c["T"]), seed=seed, scale=c.get("xscale", BIG_X) if big else 1.0)}
    if k == "chunk":
        d = {"x%d" % j: weights.synth_tensor((c["C"], 2050, L), seed=seed + j, scale=BIG_X if big else 1.0) for j, L in enumerate(c["L"])}
        d["s"] = weights.synth_tensor((4, 2, c["C"] * K, 64), seed=seed + 9, scale=0.5)
        return d
    if k == "dual":
        return {"z": weights.synth_tensor((c["C"], c["T"], K, 64), seed=seed, scale=1e5 if big else 0.4),
                "s": weights.synth_tensor((4, 2, c["C"] * K, 64), seed=seed + 9, scale=0.5)}
    if k in ("separate", "evaluate"):
        wave = weights.synth_waveform(c["R"], c["n"], seed=seed) * (BIG_WAVE if big else 1.0)
        return {"wave": wave.astype(np.float32)}
    if k == "stream":
        return {"wave": weights.synth_waveform(c["C"], c["steps"] * 1024, seed=seed)}
    raise ValueError(k)


def run_case(m, c, arr):
    """The case's call(s) on the model `m` (cuda) -> dict of numpy outputs."""
    from speechseparation_amd.bsrnn import StreamingSeparator
    cu = {k: torch.from_numpy(a).cuda() for k, a in arr.items()}
    k = c["kind"]
    if k == "forward":
        y, mask = m.forward_with_mask(cu["x"])
        return {"y": y.cpu().numpy(), "mask": mask.cpu().numpy()}
    if k == "chunk":
        s = cu["s"]
        out = {}
        for j in range(len(c["L"])):
            y, s = m.forward_chunk(cu["x%d" % j], s)
            out["y%d" % j] = y.cpu().numpy()
        out["state"] = s.cpu().numpy()
        return out
    if k == "dual":
        z, s = m.dual_path(cu["z"], cu["s"])
        return {"z": z.cpu().numpy(), "state": s.cpu().numpy()}
    if k == "separate":
        return {"out": m.separate(cu["wave"]).cpu().numpy()}
    if k == "evaluate":
        r = m.evaluate(cu["wave"], cu["wave"] * 0.5, return_estimate=True)
        return {"out": r["x_time"].cpu().numpy()}
    if k == "stream":
        st = StreamingSeparator(m, channels=c["C"])
        outs = [st.step(cu["wave"][:, j * 1024:(j + 1) * 1024].contiguous()).cpu().numpy() for j in range(c["steps"])]
        del st
        return {"out": np.stack(outs)}
    raise ValueError(k)


def make_model(tab, w):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN(None if tab == "12" else table(tab)).eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in state_dict(tab, w).items()}, strict=True)
    return m.to("cuda")


def oracle(c, arr, dtype):
    """The float64 / float32 oracle of a case on its picked rows -> dict keyed like run_case's outputs (rows picked)."""
    from oracle import bsrnn_numpy as onp
    sd, v = state_dict(c["table"], c["w"]), table(c["table"])
    K = len(v)
    k = c["kind"]
    n_rows = c.get("C", c.get("R"))
    rows = c["rows"] if c["rows"] is not None else list(range(n_rows))
    sidx = np.concatenate([np.arange(r * K, (r + 1) * K) for r in rows])
    if k == "forward":
        taps = {}
        y = onp.forward(sd, arr["x"][rows], v, dtype, taps)
        return {"y": y, "mask": taps["mask"]}
    if k == "chunk":
        s = arr["s"][:, :, sidx]
        out = {}
        for j in range(len(c["L"])):
            out["y%d" % j], s = onp.forward_chunked(sd, arr["x%d" % j][rows], s, v, dtype)
        out["state"] = s
        return out
    if k == "dual":
        z, s = onp.dual_path(sd, arr["z"][rows].astype(dtype), arr["s"][:, :, sidx].astype(dtype), dtype)
        return {"z": z, "state": s}
    if k in ("separate", "evaluate"):
        return {"out": onp.separate(sd, arr["wave"][rows].astype(dtype), v, dtype)}
    if k == "stream":
        so = onp.StreamingOracle(sd, C=c["C"], v=v, dtype=dtype)
        w = arr["wave"]
        return {"out": np.stack([so.step(w[:, j * 1024:(j + 1) * 1024]) for j in range(c["steps"])])}
    raise ValueError(k)


def pick(c, key, a):
    """Rows `c['rows']` of a run_case output (state slabs: the rows' c*K + k entries; streaming: dim 1)."""
    if c["rows"] is None:
        return a
    rows = c["rows"]
    if key == "state":
        K = len(table(c["table"]))
        return a[:, :, np.concatenate([np.arange(r * K, (r + 1) * K) for r in rows])]
    return a[:, rows] if c["kind"] == "stream" else a[rows]


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def shape_text(c):
    if "T" in c:
        return "C=%d T=%d" % (c["C"], c["T"])
    if "L" in c:
        return "C=%d L=%s" % (c["C"], "+".join(map(str, c["L"])))
    if "steps" in c:
        return "C=%d x %d steps" % (c["C"], c["steps"])
    return "R=%d n=%d" % (c["R"], c["n"])


CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[2])
from speechseparation_amd import _native
from test_gpu_exact_path import CASES, RERUN, inputs, run_case, make_model
mode = _native.compute_mode()
assert mode["gemm"] == "f32" and mode["lstm"] == "f32", mode
out, models = {}, {}
for c in CASES + RERUN:
    key = (c["table"], c["w"])
    if key not in models:
        models[key] = make_model(*key)
        assert models[key].mlp_flow() == "layers", key
    for k, a in run_case(models[key], c, inputs(c)).items():
        out[c["name"] + "/" + k] = a
    print("ran", c["name"], flush=True)
np.savez(sys.argv[1], **out)
'''


@pytest.fixture(scope="module")
def f32_child():
    """All cases of both parts, run once under BSRNN_GEMM=f32 BSRNN_LSTM=f32 in a child process -> {case/output: array}."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "f32.npz")
        env = dict(os.environ, PYTHONPATH=REPO, BSRNN_GEMM="f32", BSRNN_LSTM="f32")
        r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.join(REPO, "tests")], env=env, cwd=REPO,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:]
        return dict(np.load(path))


def test_exact_f32_path_at_every_call_shape(f32_child):
    """Every part-1 case: each output against the float64 oracle on the picked rows, e_hip <= 3 e_f32 + 1e-7 and < 1e-4 (e_f32: the
    float32 oracle's distance from float64 on the same rows), the criterion of test_precision_is_at_fp32_rounding_level."""
    bad = []
    for c in CASES:
        arr = inputs(c)
        r64, r32 = oracle(c, arr, np.float64), oracle(c, arr, np.float32)
        for key in r64:
            hip = pick(c, key, f32_child[c["name"] + "/" + key])
            assert hip.shape == r64[key].shape, (c["name"], key, hip.shape, r64[key].shape)
            e_hip, e_f32 = maxabs(hip, r64[key]), maxabs(r32[key], r64[key])
            ok = e_hip <= 3 * e_f32 + 1e-7 and e_hip < 1e-4
            print("exact f32 %-18s K=%-2d %-16s %-6s e_hip %.2e  e_f32 %.2e  bound %.2e%s" % (
                c["name"], len(table(c["table"])), shape_text(c), key, e_hip, e_f32, 3 * e_f32 + 1e-7, "" if ok else "  FAIL"))
            if not ok:
                bad.append((c["name"], key, e_hip, e_f32))
    assert not bad, bad


def test_range_guard_reruns_equal_the_exact_path(f32_child):
    """Default mode, inputs far beyond 65504, at the shapes where the default flow differs most from the exact one.  Per case:
    the guard trips (witness: the same call under the 'deferred' policy makes the next call raise), the result is within 2e-6 of the
    output range of the float64 oracle, equals the f32 child's result bit for bit, and an in-range call afterwards equals the
    one before (and the overlap state is unchanged)."""
    from speechseparation_amd import _native
    from speechseparation_amd._native import NativeError
    if _native.compute_mode()["gemm"] != "fp16x2":
        pytest.skip("range guard belongs to the fp16x2 mode")
    for c in RERUN:
        m = make_model(c["table"], c["w"])
        arr, small = inputs(c), inputs(c, in_range=True)
        if c.get("overlapped"):
            assert m.overlap_state() == 1
        ovl = m.overlap_state()
        before = run_case(m, c, small)
        state_in = torch.from_numpy(arr["s"]).cuda() if c["kind"] == "chunk" else None
        if state_in is not None:                          # the caller's state_in must come back unchanged
            s_copy = state_in.clone()
            y, s = m.forward_chunk(torch.from_numpy(arr["x0"]).cuda(), state_in)
            got = {"y0": y.cpu().numpy(), "state": s.cpu().numpy()}
            assert torch.equal(state_in, s_copy), c["name"]
        else:
            got = run_case(m, c, arr)
        after = run_case(m, c, small)
        assert m.overlap_state() == ovl, (c["name"], ovl, m.overlap_state())
        for k in before:
            assert np.array_equal(before[k], after[k]), (c["name"], k)
        # witness: under 'deferred' the same call is reported by the next one (evaluate re-runs whatever the policy: separate it)
        m.set_range_policy("deferred")
        try:
            if c["kind"] == "evaluate":
                m.separate(torch.from_numpy(arr["wave"]).cuda())
            else:
                run_case(m, c, arr)
            torch.cuda.synchronize()
            with pytest.raises(NativeError, match="65504"):
                run_case(m, c, small)
        finally:
            m.set_range_policy("exact")
        again = run_case(m, c, small)
        for k in before:
            assert np.array_equal(before[k], again[k]), (c["name"], k)
        r64 = oracle(c, arr, np.float64)
        line = []
        for k, ref in r64.items():
            hip = got[k]
            child = f32_child[c["name"] + "/" + k]
            same = np.array_equal(hip, child)
            e = maxabs(pick(c, k, hip), ref)
            rng = max(float(np.abs(ref).max()), 1.0)
            line.append("%s rel %.2e %s" % (k, e / rng, "bits == f32 child" if same else "BITS DIFFER (max %.2e)" % maxabs(hip, child)))
            assert np.isfinite(hip).all(), (c["name"], k)
            assert e / rng < (2e-4 if k == "state" else 2e-6), (c["name"], k, e / rng)   # (state: saturated gates, as in test_gpu_edges)
            assert same, (c["name"], k, maxabs(hip, child))
        print("re-run %-24s %-16s witness ok, follow-up unchanged, overlap %d | %s" % (c["name"], shape_text(c), ovl, "; ".join(line)))
        del m


# ---------------------------------------------------------------------------------------------------------------- aliased buffers
class Buf:
    """One device allocation; views at float offsets, each checked to lie inside it."""

    def __init__(self, nfloats):
        self.t = torch.zeros(nfloats, device="cuda")

    def at(self, off, n):
        assert 0 <= off and off + n <= self.t.numel()
        return self.t[off:off + n]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def test_aliased_outputs_are_refused_or_exact():
    """An out-of-range call whose output overlaps (exactly or partly) an input that the re-run reads: each entry point either
    refuses with BSRNN_EARG or returns the numbers of the same call with separate buffers, as include/bsrnn_hip.h states per
    entry point.  (Before the rule covered ranges, bsrnn_forward(x, y = x) returned rc 0 with the re-run's output computed from its
    own first, out-of-range output.)"""
    from speechseparation_amd import _native, weights
    from speechseparation_amd.bsrnn import _stream_ptr
    if _native.compute_mode()["gemm"] != "fp16x2":
        pytest.skip("range guard belongs to the fp16x2 mode")
    lib = _native.lib
    m = make_model("12", "default")
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = m._context(dev)
    s = _stream_ptr(dev)
    K = len(m.band_widths)
    C, T = 2, 6
    nx, ns, nz = C * 2050 * T, 4 * 2 * C * K * 64, C * T * K * 64
    x = torch.from_numpy(weights.synth_tensor((C, 2050, T), seed=71, scale=BIG_X)).cuda().reshape(-1)
    st = torch.from_numpy(weights.synth_tensor((4, 2, C * K, 64), seed=72, scale=0.5)).cuda().reshape(-1)
    z = torch.from_numpy(weights.synth_tensor((C, T, K, 64), seed=73, scale=1e5)).cuda().reshape(-1)
    R, n = 2, 5 * 1024 + 3
    n_out = (n // 1024) * 1024
    wave = torch.from_numpy(weights.synth_waveform(R, n, seed=74) * BIG_WAVE).cuda().reshape(-1)
    results = []

    def outcome(name, rc, got, ref, expect):
        if rc == EARG:
            msg = lib.bsrnn_last_error().decode()
            res = "EARG (%s)" % msg
            ok = expect == "earg" and ("again" in msg or "re-run" in msg)
        elif rc != 0:
            res, ok = "rc %d" % rc, False
        else:
            same = bool(got) and all(torch.equal(g, r) for g, r in zip(got, ref))
            if not got:
                res = "rc 0 (not refused)"
            else:
                res = "rc 0, %s" % ("equal to the separate-buffer call" if same else "WRONG (max |diff| %.3g)" % max(
                    float((g - r).abs().max()) for g, r in zip(got, ref)))
            ok = expect == "equal" and same
        results.append((name, res, ok))
        torch.cuda.synchronize()

    # bsrnn_forward: y / mask may overlap x (re-run from the library's own copy)
    y_ref, mask_ref = torch.empty(nx, device="cuda"), torch.empty(nx, device="cuda")
    _native.check(lib.bsrnn_forward(ctx, ptr(x), ptr(y_ref), ptr(mask_ref), C, T, s))
    for name, off_y, off_m in (("forward y = x", 0, None), ("forward y partly over x", nx // 2, None), ("forward mask = x", None, 0)):
        b = Buf(3 * nx)
        xb = b.at(nx, nx)
        xb.copy_(x)
        yb = b.at(nx + off_y, nx) if off_y is not None else torch.empty(nx, device="cuda")
        mb = b.at(nx + off_m, nx) if off_m is not None else torch.empty(nx, device="cuda")
        rc = lib.bsrnn_forward(ctx, ptr(xb), ptr(yb), ptr(mb), C, T, s)
        outcome(name, rc, [yb.clone()] + ([mb.clone()] if off_y is None else []), [y_ref] + ([mask_ref] if off_y is None else []), "equal")

    # bsrnn_forward_chunk: y may overlap x; nothing may overlap state_in
    yc_ref, sc_ref = torch.empty(nx, device="cuda"), torch.empty(ns, device="cuda")
    _native.check(lib.bsrnn_forward_chunk(ctx, ptr(x), ptr(st), ptr(yc_ref), ptr(sc_ref), C, T, s))
    for name, layout, expect in (("chunk y = x", "y=x", "equal"), ("chunk state_out = state_in", "s=s", "earg"),
                                 ("chunk state_out partly over state_in", "s~s", "earg"), ("chunk y partly over state_in", "y~s", "earg")):
        b = Buf(2 * (nx + ns) + nx)
        xb, sb = b.at(0, nx), b.at(nx, ns)
        xb.copy_(x)
        sb.copy_(st)
        yb = xb if layout == "y=x" else (b.at(nx + ns // 2, nx) if layout == "y~s" else b.at(nx + 2 * ns, nx))
        so = sb if layout == "s=s" else (b.at(nx + ns // 2, ns) if layout == "s~s" else b.at(2 * nx + 2 * ns, ns))
        rc = lib.bsrnn_forward_chunk(ctx, ptr(xb), ptr(sb), ptr(yb), ptr(so), C, T, s)
        outcome(name, rc, [yb.clone(), so.clone()], [yc_ref, sc_ref], expect)

    # bsrnn_dual_path: z_out / state_out must not overlap z / state_in
    for name, layout in (("dual z_out = z", "z=z"), ("dual z_out partly over z", "z~z"), ("dual state_out partly over state_in", "s~s"),
                         ("dual state_out partly over z", "s~z")):
        b = Buf(3 * (nz + ns))
        zb, sb = b.at(0, nz), b.at(nz, ns)
        zb.copy_(z)
        sb.copy_(st)
        zo = zb if layout == "z=z" else (b.at(nz // 2, nz) if layout == "z~z" else b.at(nz + 2 * ns, nz))
        so = b.at(nz + ns // 2, ns) if layout == "s~s" else (b.at(nz // 2, ns) if layout == "s~z" else b.at(2 * nz + 2 * ns, ns))
        rc = lib.bsrnn_dual_path(ctx, ptr(zb), ptr(zo), ptr(sb), ptr(so), C, T, s)
        outcome(name, rc, [], [], "earg")

    # bsrnn_separate: wave_out must not overlap wave
    for name, off in (("separate out = wave", 0), ("separate out partly over wave", n)):
        b = Buf(R * n + n + R * n_out)
        wb = b.at(0, R * n)
        wb.copy_(wave)
        rc = lib.bsrnn_separate(ctx, ptr(wb), ptr(b.at(off, R * n_out)), R, n, s)
        outcome(name, rc, [], [], "earg")

    # bsrnn_evaluate: est_out must not overlap mix or speech (whatever the policy)
    vals = (ctypes.c_double * len(_native.METRIC_NAMES))()
    for name, which in (("evaluate est = mix", "mix"), ("evaluate est partly over speech", "speech")):
        b = Buf(2 * R * n + R * n_out)
        mb, sp = b.at(0, R * n), b.at(R * n, R * n)
        mb.copy_(wave)
        sp.copy_(wave * 0.5)
        est = mb[:R * n_out] if which == "mix" else b.at(R * n + 100, R * n_out)
        rc = lib.bsrnn_evaluate(ctx, ptr(mb), ptr(sp), R, n, ptr(est), vals, s)
        outcome(name, rc, [], [], "earg")

    # bsrnn_stream_step: chunk and out may overlap (the chunk is kept aside); two streams fed the same chunks must agree
    chunks = torch.from_numpy(weights.synth_waveform(2, 3 * 1024, seed=75)).cuda()
    big = [1.0, 3e7, 1.0]          # step 1: |x| ~ 1e9, the LSTM operands (GEMV calls: only those) far beyond 65504
    for name, off in (("stream out = chunk", 0), ("stream out partly over chunk", 700)):
        ha, hb = ctypes.c_void_p(), ctypes.c_void_p()
        _native.check(lib.bsrnn_stream_create(ctx, 2, ctypes.byref(ha)))
        _native.check(lib.bsrnn_stream_create(ctx, 2, ctypes.byref(hb)))
        try:
            for i in range(3):
                c = (chunks[:, i * 1024:(i + 1) * 1024] * big[i]).contiguous().reshape(-1)
                ref = torch.empty(2048, device="cuda")
                _native.check(lib.bsrnn_stream_step(ha, ptr(c), ptr(ref), ctypes.c_float(1.0), s))
                b = Buf(2048 + 1024)
                cb = b.at(0, 2048)
                cb.copy_(c)
                ob = b.at(off, 2048)
                rc = lib.bsrnn_stream_step(hb, ptr(cb), ptr(ob), ctypes.c_float(1.0), s)
                outcome("%s (step %d)" % (name, i), rc, [ob.clone()], [ref], "equal")
        finally:
            lib.bsrnn_stream_destroy(ha)
            lib.bsrnn_stream_destroy(hb)

    # under the 'deferred' policy nothing is re-run and the buffers may alias as before (in-range input)
    m.set_range_policy("deferred")
    try:
        zs = (z / 1e5 * 0.4).contiguous()
        so = torch.empty(ns, device="cuda")
        rc = lib.bsrnn_dual_path(ctx, ptr(zs), ptr(zs), ptr(st), ptr(so), C, T, s)
        results.append(("deferred: dual z_out = z accepted", "rc %d" % rc, rc == 0))
        _native.check(lib.bsrnn_sync(ctx, s))
    finally:
        m.set_range_policy("exact")
    for name, res, ok in results:
        print("aliasing %-40s %s%s" % (name, res, "" if ok else "  FAIL"))
    assert all(ok for _, _, ok in results), [r for r in results if not r[2]]


def test_separate_checks_its_out_tensor():
    """BSRNN.separate(out=...) takes only a contiguous float32 [R, (n // 1024) * 1024] tensor on the call's device: anything else
    would let the kernels write past its end or into the wrong layout."""
    from speechseparation_amd import weights
    m = make_model("12", "default")
    wave = torch.from_numpy(weights.synth_waveform(2, 3 * 1024 + 5, seed=76)).cuda()
    good = torch.empty((2, 3 * 1024), device="cuda")
    ref = m.separate(wave)
    assert torch.equal(m.separate(wave, out=good), ref)
    for bad in (torch.empty((2, 2 * 1024), device="cuda"), torch.empty((2, 4 * 1024), device="cuda"),
                torch.empty((3 * 1024, 2), device="cuda").t(), torch.empty((2, 3 * 1024), device="cuda", dtype=torch.float64),
                torch.empty((2, 3 * 1024)), torch.empty((1, 3 * 1024), device="cuda")):
        with pytest.raises(ValueError, match="out must be"):
            m.separate(wave, out=bad)
