"""GPU: the room-impulse-response augmentation (speechseparation_amd/augment.py: reverb_pairs over FirBank; train.py --rir).

reverb_pairs(chain=True) is the reference as written - m_dataset.py:110-111 convolves a1 twice - against those two chained conv1d calls in
float64; chain=False against its definition.  The bound is the criterion of tests/test_gpu_convolve.py with the float32 reference run
through the same chain (convolve_reference.ref32 of ref32's result), so the rounding of the first stage's result to float32 is in e_f32 too."""
import contextlib
import io
import math

import numpy as np
import pytest
import torch

import convolve_reference as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


@pytest.fixture(scope="module")
def setup(model):
    from speechseparation_amd.augment import FirBank
    h = [cr.decaying_noise(700, 31), cr.decaying_noise(1500, 32)]
    clips = [np.stack([cr.signal(n, 40 + 2 * i), cr.signal(n, 41 + 2 * i)]) for i, n in enumerate((3000, 5000, 2500))]
    draws = [(0, 1), None, (1, 1)]
    return FirBank(model, h), h, clips, draws


@pytest.mark.parametrize("chain", [True, False])
def test_reverb_pairs(setup, chain):
    from speechseparation_amd.augment import reverb_pairs
    bank, h, clips, draws = setup
    mixes = [torch.from_numpy(c.copy()).cuda() for c in clips]
    assert reverb_pairs(bank, mixes, draws, chain=chain) is mixes
    assert torch.equal(mixes[1].cpu(), torch.from_numpy(clips[1]))          # no draw: untouched
    for i, d in enumerate(draws):
        if d is None:
            continue
        a, got = clips[i], mixes[i].cpu().numpy()
        cr.hold_row("clip %d row 0" % i, got[0], cr.ref32(a[0], h[d[0]]), cr.ref64(a[0], h[d[0]]))
        if chain:      # a2 = conv1d(a1, rir2) of the ALREADY convolved a1
            r32 = cr.ref32(cr.ref32(a[0], h[d[0]]), h[d[1]])
            r64 = cr.ref64(cr.ref64(a[0], h[d[0]]), h[d[1]])
        else:
            r32, r64 = cr.ref32(a[1], h[d[1]]), cr.ref64(a[1], h[d[1]])
        cr.hold_row("clip %d row 1 (chain = %s)" % (i, chain), got[1], r32, r64)


def test_train_step_with_rir(tmp_path):
    """One optimizer step of 4 synthetic clips through train.py --ragged: with --rir_prob 1.0 the epoch figures are finite and differ from
    the run without --rir; with --rir_prob 0 the run prints exactly the text of the run without the flag."""
    import train
    from speechseparation_amd import audio
    rirs = tmp_path / "rirs"
    rirs.mkdir()
    audio.save_wav(str(rirs / "hall_imp_01.wav"), torch.from_numpy(np.stack([cr.decaying_noise(800, 51), cr.decaying_noise(800, 52)])), 16000)
    audio.save_wav(str(rirs / "booth_imp.wav"), torch.from_numpy(cr.decaying_noise(300, 53)[None, :]), 16000)
    audio.save_wav(str(rirs / "noise.wav"), torch.from_numpy(cr.signal(500, 54)[None, :]), 16000)          # no `imp` in the name: not a response
    texts = {}
    for tag, extra in (("plain", []), ("all", ["--rir", str(rirs), "--rir_prob", "1.0"]), ("none", ["--rir", str(rirs), "--rir_prob", "0"])):
        out = tmp_path / tag
        out.mkdir()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            train.main(["--synthetic", "4", "--seconds", "1.5", "--synthetic-weights", "0", "--ragged", "--batch_size", "4", "--outdir", str(out)] + extra)
        texts[tag] = buf.getvalue()
        print(tag, texts[tag])

    def epoch(text):
        line = [ln for ln in text.splitlines() if ln.startswith("Epoch") and "Loss" in ln][0].split()
        return float(line[3]), float(line[5])
    loss, sdr = epoch(texts["all"])
    assert math.isfinite(loss) and math.isfinite(sdr)
    assert epoch(texts["all"]) != epoch(texts["plain"])
    assert texts["none"] == texts["plain"]
