"""The checks of tests/test_gpu_stream_hops.py as plain functions, so that the same ones run in the test process and in a child process
started under another time-axis form (BSRNN_TIME_SEQ8=1, BSRNN_LSTM=f32: the knobs are read once per process).  Run as a program:
    python tests/stream_hops_cases.py <case> [<case> ...]      -> prints one line per case, exit status 0 when all hold.
Bounds: TOL and STATE_TOL of tests/test_gpu_stream_block.py - output against the oracle, and state against the oracle / output between
different call shapes."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

TOL = 1e-4
STATE_TOL = 2e-5
HOP = 1024
NFFT = 2048

# test 4: six calls of C = 8 rows, L = 40 hops, whose rows between them take every count 0 .. 40 (48 slots: the seven left over repeat
# the neighbours of the 16-frame groups and of the time kernels' 8-step input chunks), and a second call on each stream
EVERY_COUNT = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15], [16, 17, 18, 19, 20, 21, 22, 23], [24, 25, 26, 27, 28, 29, 30, 31],
               [32, 33, 34, 35, 36, 37, 38, 39], [40, 0, 15, 16, 17, 31, 33, 1]]
EVERY_COUNT_NEXT = [[3, 0, 40, 1, 17, 2, 8, 5], [1, 40, 0, 7, 16, 3, 33, 2], [2, 5, 1, 40, 0, 9, 4, 15], [0, 3, 31, 2, 40, 1, 6, 4],
                    [4, 1, 2, 0, 3, 40, 24, 8], [5, 2, 4, 3, 1, 0, 40, 32]]
OVERLAP_COUNTS = [0, 1, 15, 16, 17, 32, 31, 8]             # C = 8, 32 hops: the smallest shape the overlapped dual path takes
OVERLAP_NEXT = [32, 17, 0, 1, 16, 2, 15, 3]


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def t2n(t):
    return t.detach().cpu().numpy()


def make_model(sd, v=None):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN(v).eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}, strict=True)
    return m.to("cuda")


def blob_state(blob):
    return t2n(blob)[2 * NFFT:].reshape(4, 2, -1, 64)


def fed_with_nan(x, hops):
    """x [C, L*1024] with NaN behind every row's own hops: what a hops call must never read."""
    fed = x.clone()
    for r, h in enumerate(hops):
        fed[r, h * HOP:] = float("nan")
    return fed


def check_zero_tail(out, hops, what):
    for r, h in enumerate(hops):
        assert not bool(out[r, h * HOP:].any()), ("output behind a row's count is not zero", what, r, h)
        assert bool(torch.isfinite(out[r]).all()), ("row not finite", what, r)


# ------------------------------------------------------------------------------------------------ against the oracle
def oracle_case(sd, v, C, L, calls, seed, label=""):
    """A stream of C rows takes the hops calls of `calls` ([C] counts each, L hops per call); every row against a one-row StreamingOracle
    stepped over that row's own hops only.  -> (worst output error, worst state error)."""
    from oracle import bsrnn_numpy as onp
    from speechseparation_amd import weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    m = make_model(sd, v)
    st = StreamingSeparator(m, channels=C)
    wave = weights.synth_waveform(C, len(calls) * L * HOP, seed=seed)
    oracles = [onp.StreamingOracle(sd, C=1, v=v) for _ in range(C)]
    worst = 0.0
    for i, hops in enumerate(calls):
        x = torch.from_numpy(np.ascontiguousarray(wave[:, i * L * HOP:(i + 1) * L * HOP])).cuda()
        got = st.process_hops(fed_with_nan(x, hops), hops)
        assert tuple(got.shape) == (C, L * HOP)
        check_zero_tail(got, hops, (label, i))
        for r, h in enumerate(hops):
            for l in range(h):
                ref = oracles[r].step(t2n(x[r:r + 1, l * HOP:(l + 1) * HOP]))
                e = maxabs(t2n(got[r, l * HOP:(l + 1) * HOP]), ref[0])
                print("%s call %d row %d hop %d: output vs oracle %.3e" % (label, i, r, l, e))
                worst = max(worst, e)
                assert e < TOL, ("row against its oracle", label, i, r, l, e)
    worst_state = 0.0
    for r in range(C):
        blob = st.get_row(r)
        es = maxabs(blob_state(blob), oracles[r].state)
        print("%s row %d: state vs oracle %.3e" % (label, r, es))
        worst_state = max(worst_state, es)
        assert es < STATE_TOL, ("state against the oracle", label, r, es)
        assert maxabs(t2n(blob)[:NFFT], oracles[r].buf[0]) == 0.0, ("analysis buffer", label, r)       # raw samples
        assert maxabs(t2n(blob)[NFFT:2 * NFFT], oracles[r].prev[0]) < TOL, ("previous frame", label, r)
    return worst, worst_state


def smallest_mixed_case(sd, label="12 bands"):
    """Test 1: C = 4, L = 3, hops [3, 1, 2, 0] then [0, 2, 1, 3]."""
    return oracle_case(sd, None, 4, 3, [[3, 1, 2, 0], [0, 2, 1, 3]], seed=90, label=label)


# ------------------------------------------------------------------------------------------------ against one-row twins
def twin_case(m, C, L, first, second, seed, label="", need_overlap=False):
    """A fresh stream of C rows takes two hops calls (counts `first`, then `second`); every row against a fresh ONE-row stream given
    process() of exactly that row's hops: output within STATE_TOL, the state part of the carry within STATE_TOL, the analysis buffer
    bit for bit (raw samples).  The second call makes a wrong carry show in the output, not only in the blob."""
    from speechseparation_amd import weights
    from speechseparation_amd.bsrnn import StreamingSeparator
    st, twin = StreamingSeparator(m, channels=C), StreamingSeparator(m, channels=1)
    wave = weights.synth_waveform(C, 2 * L * HOP, seed=seed)
    xs = [torch.from_numpy(np.ascontiguousarray(wave[:, i * L * HOP:(i + 1) * L * HOP])).cuda() for i in range(2)]
    gots, blobs = [], []
    for x, hops in zip(xs, (first, second)):
        gots.append(st.process_hops(fed_with_nan(x, hops), hops))
        check_zero_tail(gots[-1], hops, label)
        blobs.append([st.get_row(r) for r in range(C)])
    if need_overlap:
        assert m.overlap_state() == 1, ("the call did not take (or fell off) the overlapped dual path", m.overlap_state())
    worst = worst_state = 0.0
    for r in range(C):
        twin.reset()
        for i, hops in enumerate((first, second)):
            h = hops[r]
            if h:
                ref = twin.process(xs[i][r:r + 1, :h * HOP].contiguous())
                e = maxabs(t2n(gots[i][r, :h * HOP]), t2n(ref[0]))
                worst = max(worst, e)
                print("%s call %d row %d (%d hops): output vs one-row twin %.3e" % (label, i, r, h, e))
                assert e < STATE_TOL, ("row against its one-row twin", label, i, r, h, e)
            tb, b = t2n(twin.get_row(0)), t2n(blobs[i][r])
            es = maxabs(b[2 * NFFT:], tb[2 * NFFT:])
            worst_state = max(worst_state, es)
            assert es < STATE_TOL, ("state against the twin's", label, i, r, h, es)
            assert np.array_equal(b[:NFFT], tb[:NFFT]), ("analysis buffer against the twin's", label, i, r, h)
            assert maxabs(b[NFFT:2 * NFFT], tb[NFFT:2 * NFFT]) < STATE_TOL, ("previous frame against the twin's", label, i, r, h)
    print("%s: worst output %.3e, worst state %.3e" % (label, worst, worst_state))
    return worst, worst_state


# ------------------------------------------------------------------------------------------------ as a program (child process)
def main(argv):
    from speechseparation_amd import weights
    sd = weights.synth_state_dict(None, seed=0)
    for case in argv:
        if case == "smallest":
            smallest_mixed_case(sd, label=case)
        elif case == "every_count":
            twin_case(make_model(sd), 8, 40, EVERY_COUNT[5], EVERY_COUNT_NEXT[5], seed=96, label=case)
        elif case == "overlap":
            twin_case(make_model(sd), 8, 32, OVERLAP_COUNTS, OVERLAP_NEXT, seed=97, label=case, need_overlap=True)
        else:
            raise SystemExit("unknown case %r" % case)
        print("case %s holds" % case)
    print("all cases hold")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
