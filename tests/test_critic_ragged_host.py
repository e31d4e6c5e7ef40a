"""CPU checks of the host side of the committed critic on a padded batch: speechseparation_amd/csrc/critic_ragged_host.h (the per-row
chains, the row -> clip table, the live and dead tiles of the two fp16x2 kernels against their definition, the one-writer property of the
dx plan, the zero-propagation argument that lets layers 4 .. 2 run on the rectangle, the workspace, the verdicts) through the small
program tests/cpp/critic_ragged_check.cpp, and the new symbols (the three calls of a batch-sized step and the layer-1 dx alone, which
the GPU tests drive) in the header, the binding list and the library.  No GPU."""
import json
import os
import re
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
WIDTHS = (1024, 128, 64, 32)
CHANNELS = (2, 7, 10, 66, 2050)
LENGTHS = ((601,), (793, 601, 603), (2584, 601))
ROWS = (1, 2, 3)


def chain(T):
    out = []
    for _ in range(4):
        T = (T - 16) // 3 + 1
        out.append(T)
    return out


def batch(I, lens, rows, order=0):
    """The command line of a batch: clip c has lens[c] frames and rows[c % len(rows)] rows."""
    per = [rows[c % len(rows)] for c in range(len(lens))]
    args = [I, max(lens), order, len(lens)]
    for t, n in zip(lens, per):
        args += [t, n]
    return args, per


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("critic_ragged") / "critic_ragged_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "critic_ragged_check.cpp"), "-o", exe],
                   check=True)

    def run(*args):
        return json.loads(subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True, text=True).stdout)
    return run


CASES = [(I, lens, rows) for I in CHANNELS for lens in LENGTHS for rows in ((1,), (2,), (3,), (2, 1, 3))]
_ids = lambda c: "%d-%s-%s" % (c[0], "_".join(map(str, c[1])), "_".join(map(str, c[2])))      # noqa: E731


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_rows_tiles_and_the_zero_propagation_argument(ask, case):
    I, lens, rows = case
    for order in (0, 1) if I % 2 == 0 else (0,):
        args, per = batch(I, lens, rows, order)
        g = ask("rows", *args)
        Tmax = max(lens)
        want = [(t, c) for c, (t, n) in enumerate(zip(lens, per)) for _ in range(n)]
        assert [(r["frames"], r["clip"]) for r in g["rows"]] == want and g["clip_wrong"] == 0
        assert g["t_tiles"] == -(-chain(Tmax)[0] // 128) and g["s_tiles"] == -(-Tmax // 369)
        for r in g["rows"]:
            T = r["frames"]
            assert r["chain"] == chain(T)
            # the definition: a frame tile is live when it holds a frame below T1_r, a position tile when it holds a position below T_r
            assert r["fwd_live"] == [bt for bt in range(g["t_tiles"]) if 128 * bt < chain(T)[0]]
            assert r["dx_live"] == [bs for bs in range(g["s_tiles"]) if 369 * bs < T]
        assert g["live_fwd"] == g["live_fwd_reported"] == sum(len(r["fwd_live"]) for r in g["rows"])
        assert g["live_dx"] == g["live_dx_reported"] == sum(len(r["dx_live"]) for r in g["rows"])
        assert g["cover_wrong"] == 0 and g["dead_covers"] == 0       # the live tiles cover exactly t < T1_r, once
        assert g["reads_behind"] == 0                                # and read nothing at or behind x[r][.][T_r]
        assert g["writers_wrong"] == 0                               # every (r, i, s < Tmax) has one writer in the dx plan
        assert g["nonzero_behind"] == 0                              # a tile that writes zeros owns no position of the row's frames
        assert g["reach_wrong"] == 0                                 # the frames that reach a position >= len_r are all >= T_out_r
        assert g["fwd_reach_wrong"] == 0                             # a valid frame reads valid positions only


def test_dead_tiles_of_the_gpu_tests_batch(ask):
    """frames (793, 601, 603), rows (2, 1, 3), Tmax 793: three frame tiles per row, two of them dead for the four short rows (T1 = 196);
    three position tiles, one of them dead for those rows."""
    args, _ = batch(66, (793, 601, 603), (2, 1, 3))
    g = ask("rows", *args)
    assert g["t_tiles"] == 3 and g["s_tiles"] == 3
    assert [len(r["fwd_live"]) for r in g["rows"]] == [3, 3, 2, 2, 2, 2] and [len(r["dx_live"]) for r in g["rows"]] == [3, 3, 2, 2, 2, 2]
    assert chain(601)[0] == 196 and chain(603)[0] == 196 and chain(793)[0] == 260


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_workspace_blocks_are_disjoint_and_the_slabs_are_the_rectangles(ask, case):
    I, lens, rows = case
    args, per = batch(I, lens, rows)
    g = ask("plan", *args)
    R, Tmax, n = sum(per), max(lens), len(lens)
    ln = chain(Tmax)
    assert g["len"] == ln
    assert (g["slabs"], g["ch_per_slab"]) == (g["rect_slabs"], g["rect_ch_per_slab"])     # csc_plan(I, R, Tmax)'s: not a function of the lengths
    r4 = lambda v: -(-v // 4) * 4                                                         # noqa: E731
    at = 0
    for l in range(4):
        assert g["off_y"][l] == at
        at += r4(R * WIDTHS[l] * ln[l])
    assert g["off_shared"] == at and g["fwd_ws"] - at >= g["slabs"] * R * 1024 * ln[0]
    assert g["fwd_ws_exact"] == g["fwd_ws"] + R * I * Tmax
    at = g["fwd_ws"]
    for off, size in [(g["off_dp"][l], R * WIDTHS[l] * ln[l]) for l in range(4)] + [(g["off_pool"], 32 * n), (g["off_max"], n)]:
        assert off == at and off % 4 == 0
        at += r4(size)
    assert g["ws"] == at
    assert g["off_xp"] == at and g["off_dxp"] == at + r4(R * I * Tmax) and g["ws_exact"] == at + 2 * r4(R * I * Tmax)
    assert (g["row_bytes"], g["clip_bytes"]) == (8, 16) and g["table_bytes"] == 8 * R + 16 * n
    # the same batch with other lengths below Tmax: the same plan
    other = list(args)
    if n > 1:
        other[6] = 601
        assert ask("plan", *other) == g


def test_verdicts(ask):
    OK, BAD_CHANNELS, NO_CLIPS, BAD_CLIP_ROWS, TOO_SHORT, TOO_LONG, MISMATCH, BAD_ORDER, ODD, TOO_LARGE = range(10)

    def why(I, R, Tmax, order, clips, grad=1):
        args = [R, grad, I, Tmax, order, len(clips)]
        for t, n in clips:
            args += [t, n]
        g = ask("why", *args)
        return g["why"], g["clip"]

    base = [(793, 2), (601, 1), (603, 3)]
    for I in CHANNELS:
        for grad in (0, 1):
            assert why(I, 6, 793, 0, base, grad) == (OK, -1)
            assert why(I, 6, 793, 1, base, grad) == ((ODD if I % 2 else OK), -1)
    assert why(0, 6, 793, 0, base)[0] == BAD_CHANNELS and why(-2, 6, 793, 0, base)[0] == BAD_CHANNELS
    assert why(66, 0, 793, 0, [])[0] == NO_CLIPS
    assert why(66, 6, 793, 0, [(793, 2), (601, 0), (603, 4)]) == (BAD_CLIP_ROWS, 1)
    assert why(66, 6, 793, 0, [(793, 2), (601, -1), (603, 5)]) == (BAD_CLIP_ROWS, 1)
    assert why(66, 6, 793, 0, [(793, 2), (601, 1), (600, 3)]) == (TOO_SHORT, 2)
    assert why(66, 6, 793, 0, [(794, 2), (601, 1), (603, 3)]) == (TOO_LONG, 0)
    assert why(66, 6, 600, 0, [(600, 6)]) == (TOO_SHORT, 0)
    assert why(66, 7, 793, 0, base) == (MISMATCH, -1) and why(66, 5, 793, 0, base) == (MISMATCH, -1)
    assert why(66, 6, 793, 2, base)[0] == BAD_ORDER and why(66, 6, 793, -1, base)[0] == BAD_ORDER
    assert why(67, 6, 793, 1, base)[0] == ODD
    assert why(1 << 20, 6, 793, 0, base)[0] == TOO_LARGE                                  # W alone
    assert why(4098, 1 << 12, 601, 0, [(601, 1 << 12)])[0] == TOO_LARGE                   # x
    assert why(66, 1, (1 << 31) - 1, 0, [(601, 1)])[0] == TOO_LARGE
    # the gradient's blocks count only when the call forms one
    assert why(4098, 400, 601, 0, [(601, 400)], grad=1)[0] == TOO_LARGE and why(4098, 400, 601, 0, [(601, 400)], grad=0)[0] == OK


def test_the_symbols_are_declared_listed_bound_and_exported():
    from speechseparation_amd import _native
    names = ("bsrnn_critic_score_ragged", "bsrnn_critic_score_grad_ragged", "bsrnn_critic_ragged_layout", "bsrnn_critic_layer1_dx_ragged")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bsrnn_hip.h")).read(), flags=re.S)
    for n in names:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in _native.SYMBOLS
        fn = getattr(_native.lib, n)
        assert fn.argtypes is not None and fn.restype is not None
    lib = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    assert set(names) <= set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))


def test_layout_call_needs_no_device():
    """bsrnn_critic_ragged_layout reports the plan of the GPU tests' batch, and refuses what the calls refuse."""
    from speechseparation_amd import _native
    from speechseparation_amd.discriminator import ragged_layout
    g = ragged_layout(66, 6, 793, (793, 601, 603), (2, 1, 3))
    assert g["frames"] == chain(793) and g["t_tiles"] == 3 and g["s_tiles"] == 3
    assert g["live_t_tiles"] == 2 * 3 + 4 * 2 and g["live_s_tiles"] == 2 * 3 + 4 * 2
    assert g["ws_score_floats"] < g["ws_floats"] < g["ws_exact_floats"] and g["table_bytes"] == 6 * 8 + 3 * 16
    for bad, word in (((793, 600, 603), "clip 1 has 600 frames"), ((794, 601, 603), "more than Tmax")):
        with pytest.raises(_native.NativeError, match=word):
            ragged_layout(66, 6, 793, bad, (2, 1, 3))
    with pytest.raises(_native.NativeError, match="sum to R"):
        ragged_layout(66, 7, 793, (793, 601, 603), (2, 1, 3))
