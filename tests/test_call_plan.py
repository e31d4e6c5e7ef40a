"""CPU checks of the call plan (speechseparation_amd/csrc/plan_host.h): which kernels a call runs, the row blocks of a batch and their
hand-over flags, the dispatch orders of the overlapped dual path, the workspace segments and the cut of a long clip into segments are
host arithmetic on the call's shape, the knobs and the chain descriptors, so the library's own code is asked here without a GPU, through
the small program tests/cpp/call_plan_check.cpp.  Every expectation is a literal or an independent computation in numpy."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
MAX_PARTS = 4
F32, FP16X2 = 0, 2                            # GemmMode / LstmMode (descriptors.h)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    d = tmp_path_factory.mktemp("call_plan")
    exe = str(d / "call_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "call_plan_check.cpp"), "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True, text=True).stdout
        return json.loads(out)
    run.dir = d
    return run


# ------------------------------------------------------------------------------------------------ the plan
DEFAULTS = dict(K=12, C=64, T=32, gemv=1, overlap=1, band_pair=1, band_parts=1, time_fused=1, seq8=-1, gemm_mode=FP16X2, lstm_mode=FP16X2,
                cus=256, exact=0, fused=1, band_pair_off=0, overlap_env=1, overlap_off=0)
ORDER = tuple(DEFAULTS)
# (what differs from DEFAULTS, the fields of the plan the row states)
TRUTH = [
    (dict(C=1, T=1), dict(gemv=1, chains=0, band="SMALL", time_fc=1, seqs=4, nwg=3, overlap=0)),
    (dict(C=2, T=4), dict(gemv=0, chains=1, band="SMALL")),
    (dict(C=3, T=3), dict(band="PAIR_PARTS")),
    (dict(K=41, C=1, T=1), dict(gemv=1, band="PAIR_PARTS")),
    (dict(C=64, T=32), dict(seqs=4, nwg=192, overlap=1)),
    (dict(C=64, T=31), dict(overlap=0)),
    (dict(C=10), dict(nwg=30, overlap=0)),
    (dict(C=11), dict(nwg=33, overlap=1)),
    (dict(C=74), dict(nwg=222, overlap=1)),
    (dict(C=75), dict(nwg=225, overlap=0)),
    (dict(C=85), dict(seqs=4, nwg=255, overlap=0)),
    (dict(C=86), dict(seqs=8, nwg=129, overlap=1)),
    (dict(T=16375), dict(overlap=1)),
    (dict(T=16376), dict(overlap=0)),
    (dict(gemv=0), dict(gemv=0)),
    (dict(overlap=0), dict(overlap=0)),
    (dict(overlap_env=0), dict(overlap=0)),
    (dict(overlap_off=1), dict(overlap=0)),
    (dict(fused=0), dict(chains=0, overlap=0)),
    (dict(exact=1), dict(exact=1, lstm_f32=1, chains=0, band="LAYERS", time_fc=0, seqs=4, overlap=0)),
    (dict(band_pair_off=1), dict(band="LAYERS", time_fc=1, overlap=0)),
    (dict(band_pair=0), dict(band="LAYERS")),
    (dict(band_parts=0), dict(band="PAIR", overlap=0)),
    (dict(C=86, time_fused=0), dict(band="PAIR", time_fc=0, seqs=4, nwg=258)),
    (dict(seq8=1), dict(seqs=8, nwg=96)),
    (dict(C=86, seq8=0), dict(seqs=4, nwg=258, overlap=0)),
    (dict(gemm_mode=F32), dict(band="PAIR", time_fc=0)),
    (dict(lstm_mode=F32), dict(band="LAYERS", time_fc=0)),
    (dict(cus=64, C=16), dict(seqs=4, nwg=48, overlap=1)),
    (dict(cus=64, C=19), dict(nwg=57, overlap=0)),
    (dict(cus=64, C=22), dict(seqs=8, nwg=33, overlap=1)),
]


@pytest.mark.parametrize("case", range(len(TRUTH)))
def test_plan_truth_table(ask, case):
    change, expect = TRUTH[case]
    args = dict(DEFAULTS, **change)
    got = ask("plan", *[args[k] for k in ORDER])
    assert {k: got[k] for k in expect} == expect, (change, got)


def test_state_size(ask):
    for C, K in ((1, 12), (2, 42), (341, 12)):
        assert ask("state", C, K) == {"state": 4 * 2 * C * K * 64, "slab": 2 * 2 * C * K * 64}


# ------------------------------------------------------------------------------------------------ long-form cuts
@pytest.mark.parametrize("n", [1025, 2047, 2048, 2049, 3072, 3172, 8192, 9215, 10240])
def test_segment_cuts(ask, n):
    T = 1 + n // 1024
    got = ask("cuts", n)
    assert got["T"] == T and sorted(int(s) for s in got["segs"]) == list(range(1, T + 1))
    idx = np.pad(np.arange(n), 1024, mode="reflect")
    for seg in range(1, T + 1):
        g = got["segs"][str(seg)]
        assert g["window_floats"] == (seg + 2) * 1024 and g["block_floats"] == seg * 1024
        assert g["frame_rows_of_3"] == ([3 * seg, 3 * (T % seg)] if T % seg else [3 * seg])
        cuts = g["cuts"]
        assert len(cuts) == -(-T // seg)
        hops = []
        for i, (ta, te, hop0, nh, lo, wl) in enumerate(cuts):
            assert (ta, te) == (i * seg, min(T, i * seg + seg)), (n, seg, i)
            used = np.concatenate([idx[1024 * t:1024 * t + 2048] for t in range(ta, te)])
            assert (lo, lo + wl - 1) == (used.min(), used.max()), (n, seg, i)
            assert wl <= (te - ta + 1) * 1024 + 1 < g["window_floats"], (n, seg, i)
            assert nh <= seg
            hops += list(range(hop0, hop0 + nh))
        assert hops == list(range(T - 1)), (n, seg)
    assert n <= got["segs"][str(T)]["window_floats"]      # a one-segment clip fits one staging window


# ------------------------------------------------------------------------------------------------ row blocks
@pytest.mark.parametrize("R", [127, 128, 170, 171, 172, 255, 256, 341])
def test_row_blocks(ask, R):
    for T in (11, 12, 16, 63):
        got = ask("blocks", 12, 256, R, T)
        parts = 2 if R >= 171 and R * T >= 2048 else 1
        assert got["parts"] == parts, (R, T, got)
        r0 = got["r0"]
        assert r0[0] == 0 and r0[-1] == R and len(r0) == parts + 1 and all(b > a for a, b in zip(r0, r0[1:])), (R, T, got)
        assert got["ms"] == [(b - a) * T for a, b in zip(r0, r0[1:])], (R, T, got)
    assert ask("blocks", 12, 256, 171, 11)["parts"] == 1 and ask("blocks", 12, 256, 171, 12)["parts"] == 2


@pytest.mark.parametrize("parts", [2, 3, 4])
def test_flag_placement(ask, parts):
    got = ask("flags", parts, 40, 40)
    assert got["max_parts"] == MAX_PARTS
    cases = {(c["R"], c["T"]): c for c in got["cases"]}
    assert sorted(cases) == [(R, T) for R in range(2, 41) for T in range(1, 41)]
    for (R, T), c in cases.items():
        r0 = [R * j // parts for j in range(parts + 1)]
        assert c["r0"] == r0
        ranges = []
        for j in range(parts):
            M = (r0[j + 1] - r0[j]) * T
            assert c["offset"][j] == 2 * (r0[j] * T // 16 + j) and c["used"][j] == 2 * -(-M // 16), (R, T, j, c)
            ranges.append((c["offset"][j], c["offset"][j] + 2 * -(-M // 16)))
        for a in range(parts):
            for b in range(a + 1, parts):
                assert ranges[a][1] <= ranges[b][0] or ranges[b][1] <= ranges[a][0], (R, T, a, b, ranges)
        assert c["share"] == [0] * (parts - 1), (R, T, c)
        assert c["reserved"] == R * T // 8 + 2 * MAX_PARTS + 64
        assert max(hi for _, hi in ranges) <= c["reserved"], (R, T, ranges, c["reserved"])


# ------------------------------------------------------------------------------------------------ dispatch orders
def ready_of(m0, rows, M, T):
    """The last frame that frame rows [m0, m0 + rows) of M = C * T need from the time-axis launch (row m = batch row * T + frame)."""
    m1 = min(M - 1, m0 + rows - 1)
    return T - 1 if m0 // T != m1 // T else m1 % T


@pytest.mark.parametrize("table", ["default", "41"])
def test_overlap_dispatch_orders(ask, table):
    from speechseparation_amd import spec, weights
    v = spec.variant_bandsplits(table)
    wfile = str(ask.dir / ("weights_%s.bsrnnw" % table))
    weights.save_flat(wfile, weights.synth_state_dict(v, seed=100), v)
    cus = 256
    for C, T, nwg in ((64, 32, 192), (86, 32, 129), (3, 40, 9)):
        M = C * T
        got = ask("orders", wfile, C, T, nwg, cus)
        assert got["stride"] == got["head"] + -(-nwg // 16) * 16 and got["head"] == 16
        # band order
        order = got["band_order"]
        tiles = -(-M // 16)
        assert len(order) % 8 == 0 and len(order) - tiles < 8
        assert sorted(order[:tiles]) == list(range(tiles)) and order[tiles:] == [-1] * (len(order) - tiles)
        ready = [ready_of(16 * t, 16, M, T) for t in order[:tiles]]
        if (C, T) == (3, 40):
            assert ready_of(32, 16, M, T) == T - 1          # tile 2 (rows 32 .. 47) straddles batch rows 0 and 1
        for (ra, ta), (rb, tb) in zip(zip(ready, order), zip(ready[1:], order[1:])):
            assert ra < rb or (ra == rb and ta < tb), (table, C, T)
        # mask order
        rows, const = got["rows"], got["constant"]
        base = [(d, r) for d in range(len(rows)) for r in range(0, M, rows[d])]
        mask = list(zip(got["mask_tasks"][0::2], got["mask_tasks"][1::2]))
        assert sorted(mask) == sorted(base) and len(set(mask)) == len(base), (table, C, T)

        def rdy(t):
            return ready_of(t[1], rows[t[0]], M, T)
        cand = [t for t in base if not const[t[0]] and rows[t[0]] <= 80 and rdy(t) < T - 1]
        n_early = min(len(cand), max(0, cus - nwg))
        early, rest = mask[:n_early], mask[n_early:]
        assert all(t in cand for t in early), (table, C, T)
        assert [rdy(t) for t in early] == sorted(rdy(t) for t in early), (table, C, T)
        # ... the earliest-ready candidates, equal ones in base order: the stable sort of the candidates by readiness
        assert early == sorted(cand, key=rdy)[:n_early], (table, C, T)
        assert rest == [t for t in base if t not in set(early)], (table, C, T)


# ------------------------------------------------------------------------------------------------ workspace layout
@pytest.mark.parametrize("rows", [1, 63, 64, 4096])
def test_workspace_segments(ask, rows):
    from speechseparation_amd import spec
    v = spec.variant_bandsplits("default")
    K = len(v)
    LDA = sum((max(2 * w, 128) + 31) // 32 * 32 for w in v)       # band_columns (commit_host.h): activation rows, band-padded spectrum rows
    LDP = max(sum((2 * w + 7) // 8 * 8 for w in v), 8)
    sizes = ask("workspace", rows, LDP, LDA, K)["sizes"]

    def seg(n):
        return -(-n // 64) * 64
    assert len(sizes) == 11 and all(s % 64 == 0 for s in sizes)
    KH = K * 64
    assert sizes[:10] == [seg(rows * n) for n in (LDP, LDP, LDA, LDA, LDP, KH, KH, 2 * KH, 2 * KH, KH)]
    assert sizes[10] == seg(rows // 8 + 2 * MAX_PARTS + 64)
