"""CPU checks of the host side of the committed critic's gradient: the index arithmetic of speechseparation_amd/csrc/critic_grad_host.h
(the dx image's index map, the ownership of every input position, the fold's frame sets, the row map, the workspace, the scale rule, the
verdicts) through the small program tests/cpp/critic_grad_check.cpp.  No GPU."""
import json
import os
import struct
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
WIDTHS = (1024, 128, 64, 32)
CHANNELS = (2, 7, 10, 66, 2050, 4098)
FRAMES = (601, 602, 603, 793, 2584)
ROWS = (1, 3)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("critic_grad") / "critic_grad_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "critic_grad_check.cpp"), "-o", exe],
                   check=True)

    def run(*args):
        return json.loads(subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True, text=True).stdout)
    return run


@pytest.mark.parametrize("I", CHANNELS)
def test_dx_image_index_map_is_a_bijection_and_padding_is_zero(ask, I):
    g = ask("image", I)
    i_pad = -(-I // 8) * 8
    assert g["i_pad"] == i_pad and g["block"] == 4096 and g["halves"] == (i_pad // 8) * 64 * 4096
    assert g["twice"] == 0 and g["out_of_range"] == 0 and g["inverse_wrong"] == 0         # one-to-one, and the commit kernel's inverse agrees
    assert g["padding"] == g["halves"] - 1024 * I * 16 * 2 == 2 * 1024 * 16 * (i_pad - I)  # onto everything but the padding channels ...
    assert g["padding_not_zero"] == 0                                                     # ... which the inverse reports as zeros
    assert g["unaligned"] == 0                                                            # a lane's 8 output channels: one aligned 16-byte unit


SHAPES = [(I, C, T) for I in CHANNELS for T in FRAMES for C in ROWS]
_ids = lambda s: "-".join(str(v) for v in s)                                              # noqa: E731


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_every_position_has_one_owner_and_the_fold_is_the_definition(ask, shape):
    I, C, T = shape
    g = ask("tiles", *shape)
    assert g["i_tiles"] == -(-I // 8) and g["s_tiles"] == -(-T // 369)
    assert g["twice"] == 0 and g["not_once"] == 0 and g["tile_of_wrong"] == 0             # in both row orders (the map is a permutation)
    assert g["fold_wrong"] == 0 and g["column_outside"] == 0                              # taps and frames of every s < T, in tap order


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_workspace_blocks_are_disjoint(ask, shape):
    I, C, T = shape
    g = ask("plan", *shape)
    ln = []
    t = T
    for _ in range(4):
        t = (t - 16) // 3 + 1
        ln.append(t)
    assert g["len"] == ln and (g["ch"], g["tile_s"], g["tile_t"], g["halo"]) == (8, 369, 128, 5)
    r4 = lambda v: -(-v // 4) * 4                                                         # noqa: E731
    blocks = [(g["off_dp"][l], C * WIDTHS[l] * ln[l]) for l in range(4)] + [(g["off_pool"], 32), (g["off_max"], 1)]
    at = g["fwd_ws"]                                                                      # behind everything the forward owns
    for off, n in blocks:
        assert off == at and off % 4 == 0
        at += r4(n)
    assert g["ws"] == at
    assert g["off_xp"] == at and g["off_dxp"] == at + r4(C * I * T) and g["ws_exact"] == at + 2 * r4(C * I * T)
    # a layer's dy waits in the forward's shared block, which holds at least the largest of them
    assert g["fwd_ws"] - g["off_shared"] >= C * 1024 * ln[0]
    assert g["image_halves"] == -(-I // 8) * 64 * 4096
    assert ask("plan", *shape) == g                                                       # a function of the shape only


def test_tile_count_at_the_flagship_shape(ask):
    g = ask("tiles", 4098, 2, 601)
    assert g["i_tiles"] * g["s_tiles"] * 2 == 2052                                        # one workgroup each, over the whole K: no partial sums


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def test_scale_exponent_puts_the_maximum_into_2_14_2_15(ask):
    for v in (1.0, 1.5, 1.9999999, 2.0, 3e-6, 1e-8, 65504.0, 1e-38, 1e-40, 1.4e-45, 3e38):
        e = ask("scale", _bits(v))["e"]
        f = struct.unpack("<f", struct.pack("<f", v))[0]                                  # the fp32 value
        assert 2.0 ** 14 <= f * 2.0 ** e < 2.0 ** 15, (v, e)
    assert ask("scale", 0)["e"] == 0                                                      # a zero maximum: dx = 0 whatever the scale
    assert ask("scale", 0x7f800000)["e"] == 0 and ask("scale", 0x7fc00000)["e"] == 0      # infinity, NaN: the guard's business


def test_verdicts(ask):
    OK, BAD_CHANNELS, BAD_ROWS, TOO_SHORT, BAD_ORDER, ODD, TOO_LARGE = range(7)
    why = lambda *a: ask("why", *a)["why"]                                                # noqa: E731
    for I in CHANNELS:
        for T in FRAMES:
            for C in ROWS:
                assert why(I, C, T, 0) == OK
                assert why(I, C, T, 1) == (ODD if I % 2 else OK)
    assert why(0, 2, 601, 0) == BAD_CHANNELS and why(-3, 2, 601, 0) == BAD_CHANNELS
    assert why(66, 0, 601, 0) == BAD_ROWS
    assert why(66, 2, 600, 0) == TOO_SHORT and why(66, 2, 15, 0) == TOO_SHORT
    assert why(66, 2, 601, 2) == BAD_ORDER and why(66, 2, 601, -1) == BAD_ORDER
    assert why(67, 2, 601, 1) == ODD and why(67, 2, 601, 0) == OK
    assert why(1 << 20, 2, 601, 0) == TOO_LARGE                                           # W alone
    assert why(4098, 1 << 12, 601, 0) == TOO_LARGE                                        # x
    assert why(66, 2, 1 << 31, 0) == TOO_LARGE
    assert why(66, 1 << 20, 601, 0) == TOO_LARGE                                          # dp1
    # the two planar copies of the exact chain count: 3 x C * I * T floats pass the limit where x alone does not
    assert why(4098, 400, 601, 0) == TOO_LARGE and 400 * 4098 * 601 < (1 << 31) - 1
