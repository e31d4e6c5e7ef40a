"""Band tables beyond the two shipped ones.  bsrnn_create accepts any table of 1..256 non-negative widths summing to 1025, and
almost every shape decision of the hot path is made from the widths: the geometry of each band's fused MLP chains (rows per
workgroup, MFMA shape, the ragged split; or the per-layer flow for the whole model once a band is wider than 384 bins), the
band-block kernel for short band sequences (K <= 16), the time-axis kernel's sequences per workgroup and the overlap decision
(both from C * K).  These tests run synthetic tables that reach every geometry class and the band-count edges against the numpy
oracle, and prove what they reached through the library's own geometry query (bsrnn_chain_geometry)."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO

pytestmark = pytest.mark.gpu

N_BINS = 1025
EXTRA_WIDTHS = (449, 512, 513, 640, 767, 768, 769, 833, 1000, 1024, 1025)
CLASS_EDGES = (64, 96, 144, 192, 288, 384)       # the width ranges of the chain geometries end here (include/bsrnn_hip.h)
RAG_PAIRS = tuple(w for w in range(145, 259) if 1 <= (2 * w) % 32 <= 4)   # the ragged split under BSRNN_CHAIN_NO48 (csrc/commit_host.h)
# the 48-row class (289 - 383 bins) at whole tiles of 16: 2 w % 32 == 16 leaves one tile of 16 between a layer's output and the next
# layer's K loop (pad zeroing on), 2 w % 32 == 0 leaves none (off)
WIDTHS_48 = tuple(range(296, 384, 8))


def sweep_widths():
    """Widths 1..400 and EXTRA_WIDTHS.  Every width next to a class edge, 1..16, the ragged-split pairs and the 48-row widths at
    whole tiles of 16; the interiors of the classes every ninth width (the whole range 1..400 is 80 200 bins, 79 tables: minutes of oracle time)."""
    keep = set(range(1, 17)) | set(EXTRA_WIDTHS) | set(RAG_PAIRS) | set(WIDTHS_48)
    for w in range(1, 401):
        if any(e - 1 <= w <= e + 2 for e in CLASS_EDGES) or w % 9 == 3:
            keep.add(w)
    return sorted(keep)


def pack(widths):
    """First-fit decreasing into tables of 1025 bins, the bands of at most 384 bins apart from the wider ones (a table with one
    wider band runs the per-layer flow for all of its bands); each table is topped up with bands of at most 384 bins and ends with
    the zero-width band, as generate_bandsplits() does."""
    def ffd(ws):
        bins = []
        for w in sorted(ws, reverse=True):
            for b in bins:
                if sum(b) + w <= N_BINS:
                    b.append(w)
                    break
            else:
                bins.append([w])
        return bins
    out = []
    for t in ffd([w for w in widths if w <= 384]) + ffd([w for w in widths if w > 384]):
        r = N_BINS - sum(t)
        while r > 0:
            t.append(min(r, 384))
            r -= min(r, 384)
        out.append(t + [0])
    return out


SWEEP = pack(sweep_widths())
# both edges and one interior width of every class of the default geometry, then wider than the fused kernel takes
REPRESENTATIVE = pack([1, 40, 64, 65, 80, 96, 97, 120, 144, 145, 170, 191, 192, 193, 250, 288, 289, 296, 314, 383, 384]) + [[385, 640, 0], [1025, 0]]
MULS = (1.25, 1.5, 3, 4, 8)


def mul_table(mul):
    from speechseparation_amd import spec
    return spec.generate_bandsplits(mul=mul)[0]


def synth(v, i):
    """Seeded weights for table i: the default set for even i, the saturating lstm_gain = 3 set for odd i."""
    from speechseparation_amd import weights
    return weights.synth_state_dict(v, seed=100 + i, lstm_gain=3.0 if i % 2 else 1.0)


def make_model(sd, v, env=None):
    """A model whose context is created (and committed) under the environment `env` (BSRNN_OVERLAP is read per context)."""
    from speechseparation_amd.bsrnn import BSRNN
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        m = BSRNN(v).eval()
        m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}, strict=True)
        m = m.to("cuda")
        m._context(torch.device("cuda", torch.cuda.current_device()))
    finally:
        for k, a in old.items():
            if a is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = a
    return m


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def t2n(t):
    return t.detach().cpu().numpy()


def geometry_label(g, w):
    """Class name of a bsrnn_chain_geometry answer for a band of w bins."""
    rows, shape, rt, nw, rag, zpad = g
    if rows == -1:
        return "per-layer flow"
    if rows == 0:
        return "zero-width band"
    if shape == 32:
        return "32x32 RT%d/GR%d%s" % (rt, 8 // nw, " rag" if rag else "")
    return "16x16 %d rows%s" % (rows, ", pad-zeroed" if zpad else "")


def geometries(m, v):
    """{chain: [label per band]} through the library's query; checks the query's answers are consistent with mlp_flow()."""
    fused = m.mlp_flow() == "fused"
    out = {}
    for ch in (0, 1):
        labels = []
        for b, w in enumerate(v):
            g = m.chain_geometry(ch, b)
            if not fused:
                assert g == (-1,) * 6, (ch, b, g)
            elif w == 0:
                assert g == (0,) * 6, (ch, b, g)
            else:
                assert g[0] in (32, 48, 64, 80, 128, 256) and g[1] in (16, 32), (ch, b, g)
            labels.append(geometry_label(g, w))
        out[ch] = labels
    return out


# every class of the default knobs (include/bsrnn_hip.h, bsrnn_chain_geometry), in both chains
DEFAULT_CLASSES = {"32x32 RT1/GR8", "32x32 RT1/GR4", "32x32 RT2/GR2", "16x16 64 rows, pad-zeroed", "16x16 80 rows", "16x16 48 rows",
                   "16x16 48 rows, pad-zeroed", "per-layer flow", "zero-width band"}


class Worst:
    """Worst error per (chain, class) of the bands of a table: every band's class gets the table's error."""

    def __init__(self):
        self.d = {}

    def add(self, geo, err):
        for ch, labels in geo.items():
            for lab in set(labels):
                k = (ch, lab)
                self.d[k] = max(self.d.get(k, 0.0), err)

    def report(self, title):
        print(title)
        for ch in (0, 1):
            for (c, lab), e in sorted(self.d.items()):
                if c == ch:
                    print("  %s chain  %-32s worst %.2e" % ("split" if ch == 0 else "mask ", lab, e))

    def classes(self, ch):
        return {lab for (c, lab) in self.d if c == ch}


def test_width_sweep_against_the_oracle():
    """Every sweep table: forward (output and mask) at C = 2, T = 5 against the float64 oracle at the fp32-rounding-level criterion of
    test_precision_is_at_fp32_rounding_level, and a one-frame forward_recurrent (GEMV path) with a random state.  The tables must reach
    every geometry class in both chains, and a band wider than 384 bins must put the model on the per-layer flow."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    worst = Worst()
    seen48 = {}
    for i, v in enumerate(SWEEP):
        assert sum(v) == N_BINS and v[-1] == 0
        sd = synth(v, i)
        m = make_model(sd, v)
        geo = geometries(m, v)
        assert (m.mlp_flow() == "layers") == (max(v) > 384), v
        for b, w in enumerate(v):
            if w in WIDTHS_48 and m.mlp_flow() == "fused":
                seen48.setdefault(w, set()).update(m.chain_geometry(ch, b) for ch in (0, 1))
        x = weights.synth_tensor((2, 2050, 5), seed=200 + i, scale=1.0)
        taps64, taps32 = {}, {}
        y64 = onp.forward(sd, x, v, np.float64, taps64)
        y32 = onp.forward(sd, x, v, np.float32, taps32)
        y, mask = m.forward_with_mask(torch.from_numpy(x).cuda())
        e = 0.0
        for name, hip, r64, r32 in (("y", t2n(y), y64, y32), ("mask", t2n(mask), taps64["mask"], taps32["mask"])):
            e_hip, e_f32 = maxabs(hip, r64), maxabs(r32, r64)
            assert e_hip <= 3 * e_f32 + 1e-7 and e_hip < 1e-4, (v, name, e_hip, e_f32)
            e = max(e, e_hip)
        x1 = weights.synth_tensor((2, 2050), seed=300 + i, scale=1.0)
        s1 = weights.synth_tensor((4, 2, 2 * len(v), 64), seed=400 + i, scale=0.5)
        r1, rs = onp.forward_recurrent(sd, x1, s1, v, np.float64)
        y1, ns = m.forward_recurrent(torch.from_numpy(x1).cuda(), torch.from_numpy(s1).cuda())
        e_y, e_s = maxabs(t2n(y1), r1), maxabs(t2n(ns), rs)
        assert e_y < 1e-4 and e_s < 2e-5, (v, e_y, e_s)
        worst.add(geo, max(e, e_y))
        del m
    worst.report("width sweep: %d tables, forward |hip - f64 oracle| per geometry class" % len(SWEEP))
    for ch in (0, 1):
        missing = DEFAULT_CLASSES - worst.classes(ch)
        assert not missing, (ch, sorted(missing))
    # the 48-row widths at whole tiles of 16 ran fused, and the library zeroes the image's pad k-units exactly where a layer's output
    # (whole tiles of 16) ends short of the next layer's K loop (whole k-steps of 32)
    for w in WIDTHS_48:
        assert seen48.get(w) == {(48, 16, 3, 8, 0, int((2 * w) % 32 != 0))}, (w, seen48.get(w))


def ragged_tables():
    return [(v, "class") for v in REPRESENTATIVE] + [(mul_table(mul), "mul=%g" % mul) for mul in MULS]


def test_ragged_rows_per_class():
    """C = 3 x T = 47: 141 frame rows, ragged against the 48, 64, 80, 128 and 256 rows per workgroup of the classes.  The class edge
    tables and the reference's own generate_bandsplits(mul) tables: forward against the f64 oracle (rounding level), forward_chunk
    with a state, and separate() once."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    worst = Worst()
    for i, (v, what) in enumerate(ragged_tables()):
        sd = synth(v, i)
        m = make_model(sd, v)
        geo = geometries(m, v)
        x = weights.synth_tensor((3, 2050, 47), seed=500 + i, scale=1.0)
        y64 = onp.forward(sd, x, v, np.float64)
        y32 = onp.forward(sd, x, v, np.float32)
        y = t2n(m(torch.from_numpy(x).cuda()))
        e_hip, e_f32 = maxabs(y, y64), maxabs(y32, y64)
        assert e_hip <= 3 * e_f32 + 1e-7 and e_hip < 1e-4, (what, v, e_hip, e_f32)
        xc = np.ascontiguousarray(x[:, :, :11])
        s0 = weights.synth_tensor((4, 2, 3 * len(v), 64), seed=600 + i, scale=0.5)
        rc, rs = onp.forward_chunked(sd, xc, s0, v, np.float64)
        yc, sc = m.forward_chunk(torch.from_numpy(xc).cuda(), torch.from_numpy(s0).cuda())
        e_c, e_s = maxabs(t2n(yc), rc), maxabs(t2n(sc), rs)
        assert e_c < 1e-4 and e_s < 2e-5, (what, v, e_c, e_s)
        worst.add(geo, max(e_hip, e_c))
        print("%-8s K=%3d %-6s forward %.2e (f32 oracle %.2e)  chunk %.2e  state %.2e" % (what, len(v), m.mlp_flow(), e_hip, e_f32, e_c, e_s))
        if what == "mul=1.5":
            wave = weights.synth_waveform(2, 6 * 1024 + 5, seed=700)
            out = t2n(m.separate(torch.from_numpy(wave).cuda()))
            e_w = maxabs(out, onp.separate(sd, wave, v))
            print("mul=1.5 separate: %.2e" % e_w)
            assert e_w < 1e-4
        del m
    worst.report("141 frame rows: |hip - f64 oracle| per geometry class")
    for ch in (0, 1):
        assert {"32x32 RT2/GR2", "16x16 48 rows, pad-zeroed", "16x16 64 rows, pad-zeroed", "16x16 80 rows", "per-layer flow"} <= worst.classes(ch)


BAND_COUNT_TABLES = {
    "K=1": [1025],
    "K=2 zero last": [1025, 0],
    "K=2 zero first": [0, 1025],
    "K=16": [64] * 14 + [129, 0],
    "K=17": [64] * 15 + [65, 0],
    "K=256": [4] * 254 + [9, 0],
    "zero first": [0, 341, 342, 342],
    "zero middle": [341, 342, 0, 342],
    "zero twice": [341, 0, 342, 0, 342],
    "no zero band": [341, 342, 342],
}


@pytest.mark.parametrize("name", list(BAND_COUNT_TABLES))
def test_band_count_edges(name):
    """K = 1, 2, 16 / 17 (the band-block kernel for short band sequences ends at 16), 256 (the largest table bsrnn_create takes) and
    the zero-width band first, in the middle, twice or absent: forward_chunk with a state at C * T <= 8 (GEMV layers, small band block)
    and > 8, three streaming steps against the streaming oracle; at K = 256 also a call of C * K > 1024 time-axis sequences (eight
    sequences per workgroup)."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    v = BAND_COUNT_TABLES[name]
    assert sum(v) == N_BINS
    i = list(BAND_COUNT_TABLES).index(name)
    sd = synth(v, i)
    m = make_model(sd, v)
    geometries(m, v)
    K = len(v)
    for C, L in ((2, 3), (3, 5)):
        x = weights.synth_tensor((C, 2050, L), seed=800 + 10 * i + C, scale=1.0)
        s0 = weights.synth_tensor((4, 2, C * K, 64), seed=900 + 10 * i + C, scale=0.5)
        ry, rs = onp.forward_chunked(sd, x, s0, v, np.float64)
        y, s = m.forward_chunk(torch.from_numpy(x).cuda(), torch.from_numpy(s0).cuda())
        e_y, e_s = maxabs(t2n(y), ry), maxabs(t2n(s), rs)
        print("%s: forward_chunk C=%d L=%d: y %.2e state %.2e" % (name, C, L, e_y, e_s))
        assert e_y < 1e-4 and e_s < 2e-5, (C, L, e_y, e_s)
    st = StreamingSeparator(m, channels=2)
    so = onp.StreamingOracle(sd, C=2, v=v)
    wave = weights.synth_waveform(2, 3 * 1024, seed=1000 + i)
    for k in range(3):
        c = np.ascontiguousarray(wave[:, k * 1024:(k + 1) * 1024])
        e = maxabs(t2n(st.step(torch.from_numpy(c).cuda())), so.step(c))
        assert e < 1e-4, (k, e)
    del st
    if K == 256:
        x = weights.synth_tensor((5, 2050, 3), seed=1100, scale=1.0)          # 1280 time-axis sequences: eight per workgroup
        y64 = onp.forward(sd, x, v, np.float64)
        y32 = onp.forward(sd, x, v, np.float32)
        e_hip, e_f32 = maxabs(t2n(m(torch.from_numpy(x).cuda())), y64), maxabs(y32, y64)
        print("K=256, C=5: forward %.2e (f32 oracle %.2e)" % (e_hip, e_f32))
        assert e_hip <= 3 * e_f32 + 1e-7 and e_hip < 1e-4


def test_more_than_256_bands_is_refused():
    from speechseparation_amd import _native
    lib = _native.lib
    for v, rc in (([4] * 256 + [1], 1), ([4] * 255 + [5], 0)):
        widths = (ctypes.c_int32 * len(v))(*v)
        ctx = ctypes.c_void_p()
        assert lib.bsrnn_create(0, widths, len(v), ctypes.byref(ctx)) == rc, lib.bsrnn_last_error()
        if rc == 0:
            assert lib.bsrnn_n_bands(ctx) == 256
            lib.bsrnn_destroy(ctx)


CHILD = r'''
import json, sys, numpy as np, torch
from speechseparation_amd import weights
from speechseparation_amd.bsrnn import BSRNN
sys.path.insert(0, sys.argv[3])
from test_gpu_band_tables import synth, geometries
tables, path = json.load(open(sys.argv[1])), sys.argv[2]
full = len(sys.argv) < 5
out = {}
for i, v in tables:
    sd = synth(v, i)
    m = BSRNN(v).eval(); m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}); m = m.to("cuda")
    print("table %d flow %s geometry %s" % (i, m.mlp_flow(), json.dumps(geometries(m, v))))
    x = torch.from_numpy(weights.synth_tensor((2, 2050, 37), seed=1200 + i, scale=1.0)).cuda()
    if not full:
        out["%d_f" % i] = m(x[:, :, :5].contiguous()).cpu().numpy()
        continue
    f, mask = m.forward_with_mask(x)
    s = torch.from_numpy(weights.synth_tensor((4, 2, 2 * len(v), 64), seed=1300 + i, scale=0.5)).cuda()
    z, s = m.forward_chunk(x[:, :, :7].contiguous(), s)
    y = m.separate(torch.from_numpy(weights.synth_waveform(2, 5 * 1024 + 77, seed=1400 + i)).cuda())
    for k, a in (("f", f), ("mask", mask), ("z", z), ("s", s), ("y", y)):
        out["%d_%s" % (i, k)] = a.cpu().numpy()
    del m
np.savez(path, **out)
'''


def run_child(tables, env_extra, d, tag, full=True):
    """One process per knob set (the library reads its environment knobs once per process): the tables' outputs as an npz."""
    tpath, path = os.path.join(d, tag + ".json"), os.path.join(d, tag + ".npz")
    json.dump(tables, open(tpath, "w"))
    env = dict(os.environ, PYTHONPATH=REPO, **env_extra)
    args = [sys.executable, "-c", CHILD, tpath, path, os.path.join(REPO, "tests")] + ([] if full else ["short"])
    r = subprocess.run(args, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    geo = {}
    for line in r.stdout.splitlines():
        if line.startswith("table "):
            parts = line.split(" ", 5)
            geo[int(parts[1])] = (parts[3], {int(k): g for k, g in json.loads(parts[5]).items()})
    return geo, dict(np.load(path))


@pytest.fixture(scope="module")
def children():
    tables = list(enumerate(SWEEP))
    with tempfile.TemporaryDirectory() as d:
        res = {"layers": run_child(tables, {"BSRNN_MLP": "layers"}, d, "layers"),
               "no48": run_child(tables, {"BSRNN_CHAIN_NO48": "1", "BSRNN_CHAIN_RAG": "0"}, d, "no48"),
               "no48_rag": run_child(tables, {"BSRNN_CHAIN_NO48": "1"}, d, "no48_rag"),
               "default": run_child(tables, {}, d, "default")}
    return res


def test_fused_chains_equal_the_per_layer_flow_on_every_sweep_table(children):
    """Under BSRNN_CHAIN_NO48=1 BSRNN_CHAIN_RAG=0 every fused chain runs the 32 x 32 x 16 geometry the per-layer launches use (RT 1 / GR 1
    and RT 2 / GR 1 included): separate, forward (output and mask) and forward_chunk with state must EQUAL BSRNN_MLP=layers."""
    geo, fused = children["no48"]
    geo_l, layers = children["layers"]
    reached = {0: set(), 1: set()}
    for i, v in enumerate(SWEEP):
        assert geo_l[i][0] == "layers" and geo[i][0] == ("layers" if max(v) > 384 else "fused")
        for ch in (0, 1):
            reached[ch] |= set(geo[i][1][ch])
    for k in fused:
        assert np.array_equal(fused[k], layers[k]), k
    print("NO48, no rag: classes reached", sorted(reached[0]), sorted(reached[1]))
    for ch in (0, 1):
        assert {"32x32 RT1/GR8", "32x32 RT1/GR4", "32x32 RT2/GR2", "32x32 RT2/GR1", "32x32 RT1/GR1"} <= reached[ch], ch
        assert not any("rag" in c or "16x16" in c for c in reached[ch]), ch


@pytest.mark.parametrize("knobs", ["default", "no48_rag"])
def test_fused_chains_agree_with_the_per_layer_flow_at_rounding_level(children, knobs):
    """The 16 x 16 x 32 geometries (default) and the ragged split (BSRNN_CHAIN_NO48=1 with the split on) sum the same products in another
    order: everything agrees with BSRNN_MLP=layers to 1e-5 of the range, per table."""
    geo, fused = children[knobs]
    _, layers = children["layers"]
    reached = {0: set(), 1: set()}
    for i in range(len(SWEEP)):
        for ch in (0, 1):
            reached[ch] |= set(geo[i][1][ch])
    worst = 0.0
    for k in fused:
        rel = maxabs(fused[k], layers[k]) / np.abs(layers[k]).max()
        worst = max(worst, rel)
        assert rel < 1e-5, (k, rel)
    print("%s: fused vs per-layer flow, worst %.2e of the range" % (knobs, worst))
    if knobs == "no48_rag":
        for ch in (0, 1):
            assert "32x32 RT2/GR1 rag" in reached[ch], (ch, sorted(reached[ch]))
    else:
        for ch in (0, 1):
            assert DEFAULT_CLASSES <= reached[ch], (ch, sorted(reached[ch]))


def test_exact_f32_mode_on_the_representative_tables():
    """BSRNN_GEMM=f32 BSRNN_LSTM=f32 (the path the range guard re-runs a call on) against the f64 oracle at rounding level."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    tables = [(1000 + j, v) for j, (v, _) in enumerate(ragged_tables())]
    with tempfile.TemporaryDirectory() as d:
        geo, out = run_child(tables, {"BSRNN_GEMM": "f32", "BSRNN_LSTM": "f32"}, d, "f32", full=False)
    for i, v in tables:
        assert geo[i][0] == "layers"
        sd = synth(v, i)
        x = weights.synth_tensor((2, 2050, 37), seed=1200 + i, scale=1.0)[:, :, :5]
        y64 = onp.forward(sd, x, v, np.float64)
        y32 = onp.forward(sd, x, v, np.float32)
        e_hip, e_f32 = maxabs(out["%d_f" % i], y64), maxabs(y32, y64)
        print("f32 mode K=%d: %.2e (f32 oracle %.2e)" % (len(v), e_hip, e_f32))
        assert e_hip <= 3 * e_f32 + 1e-7 and e_hip < 1e-4, (v, e_hip, e_f32)


OVERLAP_TABLE = [1, 2, 3, 4, 6, 8, 11, 16, 20, 24, 32, 40, 48, 64, 72, 96, 110, 144, 192, 80, 50, 2, 0]    # K = 23


def test_overlapped_dual_path_on_a_23_band_table():
    """C = 6 x T = 40 at K = 23: 138 time-axis sequences, 35 workgroups - inside the overlap window.  The overlapped flow must equal
    BSRNN_OVERLAP=0 bit for bit."""
    from speechseparation_amd import weights
    v = OVERLAP_TABLE
    assert sum(v) == N_BINS
    sd = synth(v, 7)
    a, b = make_model(sd, v), make_model(sd, v, {"BSRNN_OVERLAP": "0"})
    assert a.overlap_state() == 1 and b.overlap_state() == 0
    x = torch.from_numpy(weights.synth_tensor((6, 2050, 40), seed=1500, scale=1.0)).cuda()
    ya, ma = a.forward_with_mask(x)
    yb, mb = b.forward_with_mask(x)
    assert a.overlap_state() == 1
    assert torch.equal(ya, yb) and torch.equal(ma, mb)


def test_training_gradients_on_a_mixed_table():
    """K = 14, bands of 1 to 200 bins and one of 474 bins (so the whole model runs the per-layer flow: no fused chain geometry takes
    part; the training kernels are per layer anyway): the gradients of all parameters against
    torch.autograd on the CPU restatement, at the bound of test_training_gradients_on_the_41_band_table."""
    from oracle.bsrnn_torch_cpu import TorchCpuBSRNN
    from speechseparation_amd import train, weights
    from speechseparation_amd.bsrnn import BSRNN
    v = [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 120, 200, 474, 0]
    assert sum(v) == N_BINS
    sd = synth(v, 3)
    x = torch.from_numpy(weights.synth_tensor((2, 2050, 5), seed=7, scale=1.0))
    target = torch.from_numpy(weights.synth_tensor((2, 2050, 5), seed=8, scale=1.0))
    ref = TorchCpuBSRNN(sd, v)
    params = ref.trainable()
    (ref.forward_differentiable(x) - target).abs().mean().backward()
    m = BSRNN(v).train()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd.items()})
    m = m.to("cuda:0")
    (train.forward_train(m, x.cuda()) - target.cuda()).abs().mean().backward()
    worst, n = ("", 0.0), 0
    for name, p in m.named_parameters():
        if p.numel() == 0:
            continue
        g_ref = params[name].grad
        a, b = p.grad.detach().cpu().double(), g_ref.detach().cpu().double()
        e = float((a - b).abs().max() / max(1e-30, float(b.abs().max()))) if float(b.abs().max()) > 0 else float(a.abs().max())
        worst = max(worst, (name, e), key=lambda t: t[1])
        n += 1
    print("mixed table: %d parameter tensors, worst relative gradient error %.2e (%s)" % (n, worst[1], worst[0]))
    assert n > 250 and worst[1] < 1e-3, worst
