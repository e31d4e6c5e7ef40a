"""CPU checks of the committed critic's host side: the index arithmetic of speechseparation_amd/csrc/critic_score_host.h (the fp16x2 image's
index map, the channel map of an interleaved input, the K slabs, the workspace, the verdicts) through the small program
tests/cpp/critic_score_check.cpp.  No GPU."""
import json
import os
import subprocess

import pytest
import torch

from conftest import REPO

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
WIDTHS = (1024, 128, 64, 32)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("critic_score") / "critic_score_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "critic_score_check.cpp"), "-o", exe],
                   check=True)

    def run(*args):
        return json.loads(subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True, text=True).stdout)
    return run


@pytest.mark.parametrize("I", [1, 2, 10, 66, 2050, 4098])
def test_image_index_map_is_a_bijection_and_padding_is_zero(ask, I):
    g = ask("image", I)
    i_pad = -(-I // 2) * 2
    assert g["i_pad"] == i_pad and g["block"] == 4096 and g["halves"] == 8 * i_pad * 4096
    assert g["twice"] == 0 and g["out_of_range"] == 0 and g["inverse_wrong"] == 0         # one-to-one, and the inverse the commit kernel uses agrees
    assert g["padding"] == g["halves"] - 1024 * I * 16 * 2 == 8 * (i_pad - I) * 4096    # onto everything but the padding channels ...
    assert g["padding_not_zero"] == 0                                                     # ... which the inverse reports as zeros
    assert g["unaligned"] == 0                                                            # a lane's 8 taps are one aligned 16-byte unit


@pytest.mark.parametrize("I", [2, 10, 66, 2050, 4098])
def test_interleaved_channel_map_matches_reference_channel_order(ask, I):
    from speechseparation_amd.discriminator import reference_channel_order
    rows = ask("rows", I, 1)["rows"]
    assert sorted(rows) == list(range(I))                                                 # a permutation
    y = torch.arange(I, dtype=torch.float32).reshape(1, I, 1)                            # interleaved rows, numbered
    assert rows == [int(v) for v in reference_channel_order(y).flatten()]
    assert ask("rows", I, 0)["rows"] == list(range(I))


SHAPES = [(I, C, T) for I in (1, 2, 10, 66, 2050, 4098) for C, T in ((1, 601), (2, 601), (3, 793), (2, 2813), (64, 601))]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_slabs_cover_every_channel_once_and_workspace(ask, shape):
    I, C, T = shape
    g = ask("plan", *shape)
    ln = []
    t = T
    for _ in range(4):
        t = (t - 16) // 3 + 1
        ln.append(t)
    assert g["len"] == ln and g["t_tiles"] == -(-ln[0] // 128) and g["o_tiles"] == 8
    rs = g["slab_ranges"]
    assert len(rs) == g["slabs"] >= 1 and rs[0][0] == 0 and rs[-1][1] == I
    assert all(a[1] == b[0] for a, b in zip(rs, rs[1:])) and all(lo < hi for lo, hi in rs)
    assert g["ch_per_slab"] % g["ch"] == 0 and all(hi - lo == g["ch_per_slab"] for lo, hi in rs[:-1])
    assert g["slabs"] == 1 or g["ch_per_slab"] >= g["min_slab"]
    tiles = C * g["t_tiles"] * g["o_tiles"]
    assert g["slabs"] == 1 or tiles * (g["slabs"] - 1) < g["fill"]                      # no more slabs than the fill asks for
    # workspace: the four outputs one after the other (16-byte aligned), then the shared block
    r4 = lambda v: -(-v // 4) * 4                                                         # noqa: E731
    at = 0
    for l in range(4):
        assert g["off_y"][l] == at
        at += r4(C * WIDTHS[l] * ln[l])
    assert g["off_shared"] == at
    shared = max([g["slabs"] * C * 1024 * ln[0]] + g["exact_scratch"])
    assert g["ws"] == at + r4(shared) and g["ws_exact"] == g["ws"] + C * I * T
    assert ask("plan", *shape) == g                                                       # a function of the shape only


def test_partial_last_slab_and_chip_fill(ask):
    g = ask("plan", 2050, 2, 601)                                                         # 32 tiles: 16 slabs
    assert g["slabs"] * 2 * g["t_tiles"] * 8 >= 512
    g = ask("plan", 66, 3, 793)
    assert g["slabs"] > 1 and 66 % g["ch_per_slab"] != 0                                 # the shape of the GPU tests has a partial last slab
    g = ask("plan", 4098, 2, 601)
    assert g["slab_ranges"][-1][1] - g["slab_ranges"][-1][0] <= g["ch_per_slab"]


def test_verdicts(ask):
    OK, BAD_CHANNELS, BAD_ROWS, TOO_SHORT, BAD_ORDER, ODD, TOO_LARGE = range(7)
    why = lambda *a: ask("why", *a)["why"]                                                # noqa: E731
    assert why(2050, 2, 601, 0) == OK and why(2050, 2, 601, 1) == OK and why(4098, 2, 2813, 1) == OK
    assert why(0, 2, 601, 0) == BAD_CHANNELS and why(-3, 2, 601, 0) == BAD_CHANNELS
    assert why(66, 0, 601, 0) == BAD_ROWS
    assert why(66, 2, 600, 0) == TOO_SHORT and why(66, 2, 15, 0) == TOO_SHORT
    assert why(66, 2, 601, 2) == BAD_ORDER and why(66, 2, 601, -1) == BAD_ORDER
    assert why(67, 2, 601, 1) == ODD and why(67, 2, 601, 0) == OK
    assert why(1 << 20, 2, 601, 0) == TOO_LARGE                                           # W alone
    assert why(4098, 1 << 12, 601, 0) == TOO_LARGE                                        # x
    assert why(66, 2, 1 << 31, 0) == TOO_LARGE
    assert why(66, 1 << 20, 601, 0) == TOO_LARGE                                          # y1
