"""The band-pair launch with two tiles of 16 sequences per workgroup (csrc/lstm.hip::band_pair_h2_kernel<., 2>: each layer's weights
loaded once for both tiles) against one tile per workgroup.  Same instructions on the same numbers in the same order per tile, so
everything the library returns must be EQUAL, bit for bit.  The form is fixed per process (BSRNN_BAND_PAIR=tiles1 / tiles2, read once;
unset: by the call's size, plan_host.h::band_pair_tiles), so every form runs in a child process of its own; the children run side by side
and every test reads what they saved."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

CHILD = r'''
import os, sys, numpy as np, torch
from speechseparation_amd import _native, spec, weights
from speechseparation_amd.bsrnn import BSRNN
what, path = sys.argv[1], sys.argv[2]
out = {}

def model(v=None, overlap=None):
    sd = weights.synth_state_dict(v, seed=1, lstm_gain=3.0)
    if overlap is not None:
        os.environ["BSRNN_OVERLAP"] = overlap            # (read when the context is created)
    m = BSRNN(v).eval(); m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd.items()}); m = m.to("cuda")
    m._context(torch.device("cuda", torch.cuda.current_device()))
    os.environ.pop("BSRNN_OVERLAP", None)
    return m

def taps(m, tag, R, T, seed):
    """The dual path alone on z [R, T, K, 64] (its output and the state it returns), and separate() on R rows of T frames."""
    K = len(m.band_widths)
    z = torch.from_numpy(np.random.default_rng(seed).standard_normal((R, T, K, 64)).astype(np.float32) * 0.5).cuda()
    zo, st = m.dual_path(z)
    out[tag + "_z"], out[tag + "_state"] = zo.cpu().numpy(), st.cpu().numpy()
    w = torch.from_numpy(weights.synth_waveform(R, (T - 1) * 1024 + 5, seed=seed)).cuda()
    out[tag + "_y"] = m.separate(w).cpu().numpy()

m = model()
if what == "shapes":
    taps(m, "one_tile", 2, 8, 11)                # R T = 16: one tile, B absent
    taps(m, "three_tiles", 1, 37, 12)            # 37: one pair plus a single, ragged last tile
    taps(m, "odd_ragged", 1, 16 * 17 + 5, 13)    # 277: 18 tiles, the last one ragged
    taps(m, "again", 1, 37, 12)                  # the same call a second time in this process: the flags' counts go on
    # overlapped: 12 rows x 32 frames = 24 tiles, 36 time-axis workgroups - the second band block waits tile by tile beside the first time-axis launch
    ser = model(overlap="0")
    w = torch.from_numpy(weights.synth_waveform(12, 31 * 1024 + 5, seed=14)).cuda()
    for i in range(2):
        out["overlapped_y%d" % i] = m.separate(w).cpu().numpy()
    out["serial_y"] = ser.separate(w).cpu().numpy()
    out["overlap_states"] = np.array([m.overlap_state(), ser.overlap_state()])
    v = spec.variant_bandsplits("41")
    taps(model(v), "b41", 7, 3, 15)              # the 41-band table: L = len(v) positions, 21 sequences
elif what == "mixed":
    # one context, calls of two sizes alternately: 33 x 125 = 4125 frame rows (258 tiles: more than one round of one-tile workgroups) and
    # 1 x 37 (three tiles) - their tiles 0 .. 2 share flags
    big = torch.from_numpy(weights.synth_waveform(33, 124 * 1024 + 5, seed=16)).cuda()
    small = torch.from_numpy(weights.synth_waveform(1, 36 * 1024 + 5, seed=12)).cuda()
    for i in range(2):
        out["big%d" % i] = m.separate(big).cpu().numpy()
        out["small%d" % i] = m.separate(small).cpu().numpy()
    out["last_error"] = np.array(_native.lib.bsrnn_last_error().decode("utf-8", "replace"))
    out["overlap_states"] = np.array([m.overlap_state()])
np.savez(path, **out)
'''

# child -> (what it runs, its environment)
CHILDREN = {
    "tiles1": ("shapes", {"BSRNN_BAND_PAIR": "tiles1"}),
    "tiles2": ("shapes", {"BSRNN_BAND_PAIR": "tiles2"}),
    "mixed_tiles1": ("mixed", {"BSRNN_BAND_PAIR": "tiles1"}),
    "mixed_auto": ("mixed", {}),
    "mixed_mismatch": ("mixed", {"BSRNN_BAND_PAIR": "mismatch"}),
    "mixed_layers": ("mixed", {"BSRNN_BAND_PAIR": "0"}),
}


@pytest.fixture(scope="module")
def saved():
    with tempfile.TemporaryDirectory() as d:
        procs = {}
        for name, (what, extra) in CHILDREN.items():
            env = dict(os.environ, PYTHONPATH=REPO, **extra)
            if not extra:
                env.pop("BSRNN_BAND_PAIR", None)
            procs[name] = subprocess.Popen([sys.executable, "-c", CHILD, what, os.path.join(d, name + ".npz")], env=env, cwd=REPO,
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        got = {}
        for name, p in procs.items():
            text, _ = p.communicate(timeout=600)
            assert p.returncode == 0, (name, text[-3000:])
            got[name] = dict(np.load(os.path.join(d, name + ".npz")))
    return got


def equal(a, b, keys):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("tag", ["one_tile", "three_tiles", "odd_ragged", "b41"])
def test_two_tiles_equal_one_tile_bit_for_bit(saved, tag):
    equal(saved["tiles2"], saved["tiles1"], [tag + s for s in ("_z", "_state", "_y")])
    assert np.isfinite(saved["tiles2"][tag + "_y"]).all() and np.abs(saved["tiles2"][tag + "_y"]).max() > 0


def test_the_same_call_twice_in_one_process(saved):
    """The flags of a tile count the launches over it: the second call finds them one launch on."""
    for form in ("tiles1", "tiles2"):
        g = saved[form]
        for s in ("_z", "_state", "_y"):
            equal({"v": g["again" + s]}, {"v": g["three_tiles" + s]}, ["v"])


def test_overlapped_consumer_with_two_tiles(saved):
    """The second band block as a consumer that waits for tile A's rows in front of A and for B's in front of B: equal to the serial flow
    (BSRNN_OVERLAP=0) of the same build and to one tile per workgroup, and nothing gave up."""
    for form in ("tiles1", "tiles2"):
        g = saved[form]
        assert list(g["overlap_states"]) == [1, 0], form
        for i in range(2):
            equal({"y": g["overlapped_y%d" % i]}, {"y": g["serial_y"]}, ["y"])
    equal(saved["tiles2"], saved["tiles1"], ["overlapped_y0", "serial_y"])


def test_calls_of_both_forms_alternate_in_one_context(saved):
    """Unset, a call of 4125 frame rows runs two tiles per workgroup and one of 37 runs one; they share the flags of tiles 0 .. 2.  Each call
    equals the same sequence with one tile per workgroup throughout; no guard was reported and the large call stayed overlapped."""
    auto, ref = saved["mixed_auto"], saved["mixed_tiles1"]
    equal(auto, ref, ["big0", "small0", "big1", "small1"])
    equal(auto, {"big0": auto["big1"], "small0": auto["small1"]}, ["big0", "small0"])
    assert str(auto["last_error"]) == "" and list(auto["overlap_states"]) == [1]


def test_mismatch_with_two_tiles_is_reported_and_falls_back(saved):
    """BSRNN_BAND_PAIR=mismatch (test hook): every workgroup publishes a wrong XCC id.  The first call - 4125 frame rows, two tiles per
    workgroup - reports guard value 4 (the library's message names it), runs again with one launch per layer and returns that flow's
    numbers (BSRNN_BAND_PAIR=0) with rc 0; the context stays there."""
    bad, layers = saved["mixed_mismatch"], saved["mixed_layers"]
    assert "did not find its partner workgroups" in str(bad["last_error"]), str(bad["last_error"])
    assert str(layers["last_error"]) == ""
    equal(bad, layers, ["big0", "small0", "big1", "small1"])
