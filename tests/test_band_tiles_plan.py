"""CPU checks of the rule that gives a workgroup of the band-pair launch one or two tiles of 16 sequences
(speechseparation_amd/csrc/plan_host.h: band_pair_tiles, band_pair_slots, band_pair_grid, and Flow::band_tiles of plan_call): two tiles
exactly where one tile per workgroup - 2 directions x ceil(N / 16) workgroups - exceeds the 2 x CUs resident workgroups of the launch.
Host arithmetic, asked of the library's own header through tests/cpp/band_tiles_check.cpp; every expectation is a literal or computed here."""
import json
import os
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
CUS = 256
BOUNDARY = 2 * CUS * 16 // 2            # 4096 sequences: 256 tiles x 2 directions = the 512 resident workgroups exactly


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("band_tiles") / "band_tiles_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "band_tiles_check.cpp"), "-o", exe], check=True)

    def run(*args):
        return json.loads(subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, check=True, text=True).stdout)
    return run


def expected(N, cus, tiles):
    n_tiles = -(-N // 16)
    slots = -(-n_tiles // 2) if tiles == 2 else n_tiles
    return dict(tiles=tiles, slots=slots, grid=-(-slots // 8) * 16)


@pytest.mark.parametrize("N,tiles", [(8064, 2), (8192, 2), (BOUNDARY - 16, 1), (BOUNDARY, 1), (BOUNDARY + 1, 2), (BOUNDARY + 16, 2), (37, 1), (16, 1),
                                     (8080, 2), (1, 1)])
def test_rule(ask, N, tiles):
    got = ask("rule", N, CUS, 0)
    assert got == expected(N, CUS, tiles), (N, got)
    assert tiles == (2 if 2 * -(-N // 16) > 2 * CUS else 1)
    # every tile has a place, both directions of eight slots per 16 workgroups
    assert got["slots"] * tiles >= -(-N // 16) and got["grid"] % 16 == 0 and got["grid"] // 2 >= got["slots"] > got["grid"] // 2 - 8


def test_metric_shape_is_one_dispatch_round(ask):
    """64 rows x 126 frames: 504 tiles, 1008 workgroups with one tile each (two rounds of 512); with two 504 that work, in a grid of
    whole groups of 16: 512, the resident workgroups exactly."""
    assert ask("rule", 64 * 126, CUS, 0) == dict(tiles=2, slots=252, grid=512)
    assert ask("rule", 64 * 126, CUS, 0)["grid"] <= 2 * CUS
    assert ask("rule", 64 * 126, CUS, 1) == dict(tiles=1, slots=504, grid=1008)


def test_odd_tile_count_leaves_the_last_slot_with_one_tile(ask):
    got = ask("rule", 8080, CUS, 0)                  # 505 tiles
    assert got == dict(tiles=2, slots=253, grid=512)
    got = ask("rule", 37, CUS, 2)                    # three tiles: one pair plus a single
    assert got == dict(tiles=2, slots=2, grid=16)


@pytest.mark.parametrize("N", [16, 37, 4096, 8064])
def test_forced_forms(ask, N):
    for force in (1, 2):
        assert ask("rule", N, CUS, force) == expected(N, CUS, force)


def test_other_device_sizes(ask):
    assert ask("rule", 1024, 64, 0)["tiles"] == 1 and ask("rule", 1025, 64, 0)["tiles"] == 2
    assert ask("rule", 4864, 304, 0)["tiles"] == 1 and ask("rule", 4865, 304, 0)["tiles"] == 2


@pytest.mark.parametrize("C,T,force,band,tiles", [(64, 126, 0, "PAIR_PARTS", 2), (64, 126, 1, "PAIR_PARTS", 1), (32, 126, 0, "PAIR_PARTS", 1),
                                                  (32, 128, 0, "PAIR_PARTS", 1), (33, 125, 0, "PAIR_PARTS", 2), (3, 3, 0, "PAIR_PARTS", 1),
                                                  (3, 3, 2, "PAIR_PARTS", 2), (2, 4, 2, "SMALL", 2), (1, 1, 0, "SMALL", 1)])
def test_plan_carries_the_rule(ask, C, T, force, band, tiles):
    """plan_call decides on the call's frame rows C * T; the few-sequence kernel (band SMALL) is chosen before and whatever is forced."""
    got = ask("plan", 12, C, T, CUS, force)
    assert got == dict(band=band, band_tiles=tiles), (C, T, force, got)
