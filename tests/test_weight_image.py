"""CPU checks of the committed weight image (speechseparation_amd/csrc/commit_host.h): what bsrnn_commit_params uploads - job and
tile tables, the fused chains' geometry and fragment streams, the recurrent weights in MFMA operand order - is host arithmetic on
the parameters, the band table and a few knobs, so it is built and examined here without a GPU, by the small program
tests/cpp/weight_image_check.cpp."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO
from test_gpu_band_tables import DEFAULT_CLASSES, SWEEP, WIDTHS_48, geometry_label, synth

CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
FP16X2 = 2                                    # GemmMode (descriptors.h), the default
SEGS = ("bandW0", "bandW1", "bandB0", "bandB1", "bandW16_0", "bandW16_1", "bandFc16", "bandFcB", "timeW", "timeB", "timeW16", "timeFc16",
        "timeFcB")                            # BlockSegs (commit_host.h), in the order the program prints them


@pytest.fixture(scope="module")
def weight_image(tmp_path_factory):
    d = tmp_path_factory.mktemp("weight_image")
    exe = str(d / "weight_image_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, os.path.join(REPO, "tests", "cpp", "weight_image_check.cpp"), "-o", exe], check=True)

    def run(sd, v, gemm_mode=FP16X2, mlp_layers=0, no48=0, no80=0, rag=1):
        """-> (the program's JSON answer, path of the image dump)"""
        from speechseparation_amd import weights
        wfile, dump = str(d / "weights.bsrnnw"), str(d / "image.bin")
        weights.save_flat(wfile, sd, v)
        out = subprocess.run([exe, wfile] + [str(int(a)) for a in (gemm_mode, mlp_layers, no48, no80, rag)] + [dump],
                             stdout=subprocess.PIPE, check=True, text=True).stdout
        return json.loads(out), dump
    return run


def test_sweep_tables_reach_every_chain_geometry(weight_image):
    """What test_width_sweep_against_the_oracle asserts through bsrnn_chain_geometry on the GPU, from the image alone: the sweep tables
    reach every geometry class of the default knobs in both chains, a band wider than 384 bins puts the whole model on the per-layer
    flow, and the 48-row widths at whole tiles of 16 zero the image's pad k-units exactly where a layer's output ends short of the
    next layer's K loop."""
    reached = {0: set(), 1: set()}
    seen48 = {}
    for i, v in enumerate(SWEEP):
        info, _ = weight_image(synth(v, i), v)
        assert info["fused"] == (max(v) <= 384), v
        for ch in (0, 1):
            geo = [tuple(g) for g in info["geometry"][ch]]
            assert len(geo) == len(v)
            for b, w in enumerate(v):
                if not info["fused"]:
                    assert geo[b] == (-1,) * 6, (ch, b, geo[b])
                elif w == 0:
                    assert geo[b] == (0,) * 6, (ch, b, geo[b])
                else:
                    assert geo[b][0] in (32, 48, 64, 80, 128, 256) and geo[b][1] in (16, 32), (ch, b, geo[b])
                    if w in WIDTHS_48:
                        seen48.setdefault(w, set()).add(geo[b])
                reached[ch].add(geometry_label(geo[b], w))
    for ch in (0, 1):
        missing = DEFAULT_CLASSES - reached[ch]
        assert not missing, (ch, sorted(missing))
    for w in WIDTHS_48:
        assert seen48.get(w) == {(48, 16, 3, 8, 0, int((2 * w) % 32 != 0))}, (w, seen48.get(w))


def arena_of(dump):
    with open(dump, "rb") as f:
        n = int(np.fromfile(f, "<u8", 1)[0])
        return np.fromfile(f, "<f4", n)


def check_bfrag_block(got, W, tile, bk):
    """got [2 piece][64 lane][8] fp16 is block (tile, bk) of W in the 16 x 16 x 32 MFMA's B-operand order: lane l, element e holds
    W[16 tile + (l & 15)][32 bk + 8 (l >> 4) + e], as the two pieces of test_split_formats.py (p0 = fp16(a), p1 = fp16((a - p0) 2048),
    p0 + p1 / 2048 = a to 22 bits)."""
    l, e = np.meshgrid(np.arange(64), np.arange(8), indexing="ij")
    a = W[16 * tile + (l & 15), 32 * bk + 8 * (l >> 4) + e].astype(np.float32)
    p0 = a.astype(np.float16)
    p1 = ((a - p0.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    assert np.array_equal(got.view(np.uint16), np.stack([p0, p1]).view(np.uint16)), (tile, bk)
    rec = got[0].astype(np.float64) + got[1].astype(np.float64) / 2048.0
    assert np.all(np.abs(rec - a) <= np.maximum(np.abs(a.astype(np.float64)) * 2.0 ** -22, 2.0 ** -35)), (tile, bk)


def test_bfrag16_segments_against_an_independent_index_computation(weight_image, sd_default):
    """pack_bfrag16 through its callers: the second layer of the first time-axis LSTM ([W_ih | W_hh], nothing folded), stored
    [2 layer][4 wave][4 blk][4 gate][2 piece][64 lane][8] where the tile of (wave, gate) is rows 64 gate + 16 wave .. + 15, and the fc
    layers of the first time block ([4 wave][2 blk]) and of the first band block ([4 tile][4 blk])."""
    info, dump = weight_image(sd_default, None)
    arena = arena_of(dump)
    assert arena.size == info["arena_floats"]
    seg = dict(zip(SEGS, info["segs"][0]))

    def halves(name, shape):
        n = int(np.prod(shape))
        return arena[seg[name]:seg[name] + n // 2].view(np.float16).reshape(shape)

    W = np.concatenate([sd_default["lstms.1.m.rnn.weight_ih_l1"], sd_default["lstms.1.m.rnn.weight_hh_l1"]], axis=1)
    assert W.shape == (256, 128)
    got = halves("timeW16", (2, 4, 4, 4, 2, 64, 8))[1]
    for wv in range(4):
        for bk in range(4):
            for g in range(4):
                check_bfrag_block(got[wv, bk, g], W, 4 * g + wv, bk)
    for name, key, nblk in (("timeFc16", "lstms.1.m.fc.weight", 2), ("bandFc16", "lstms.0.m.fc.weight", 4)):
        Wfc = sd_default[key]
        assert Wfc.shape == (64, 32 * nblk)
        got = halves(name, (4, nblk, 2, 64, 8))
        for tile in range(4):
            for bk in range(nblk):
                check_bfrag_block(got[tile, bk], Wfc, tile, bk)


# SHA-256 of the whole image dump (arena, jobs, tiles, slot tables, chain descriptors, segment offsets: weight_image_check.cpp) of the
# default band table with synth_state_dict(seed=100) under the default knobs.  It was recorded when the image builder moved out of
# bsrnn_commit_params, from dumps that the old and the new code produced byte for byte alike; a change to any operand layout changes it.
DEFAULT_IMAGE_SHA256 = "29b720a243fecf5db9784a3aba368269600c18e3fee3a3c800e2b01c3c68a876"


def test_default_image_is_the_recorded_one(weight_image):
    from speechseparation_amd import spec, weights
    v = spec.generate_bandsplits()[0]
    _, dump = weight_image(weights.synth_state_dict(v, seed=100), v)
    h = hashlib.sha256()
    with open(dump, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    assert h.hexdigest() == DEFAULT_IMAGE_SHA256
