"""GPU: the critic's 4096-point analysis (discriminator.critic_spectrum -> bsrnn_critic_spectrum; csrc/stft4096.hip) against the float64
evaluation of the reference's own call on the CPU, at the sizes where the kernels change behaviour.  Criterion, case table, references and
the CPU proof that a float32 evaluation of this pass structure meets the criterion: tests/test_critic_spectrum_reference.py.  Every
tolerance comes from the float32 evaluation of the reference, none from the kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import critic_reference as cr
import test_critic_spectrum_reference as cs
from test_dsp_reference import hold, waveform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOP, BINS, CH = cs.HOP, cs.BINS, cs.CH


def spectrum(w, scale=1.0):
    from speechseparation_amd.discriminator import critic_spectrum
    return critic_spectrum(w, scale)


# ------------------------------------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("R,n,signal", cs.runs())
def test_against_float64(R, n, signal):
    wave, ref32, ref64 = cs.references(R, n, signal)
    w = torch.from_numpy(wave).to(DEV)
    x = spectrum(w)
    T = cs.frames_of(n)
    assert tuple(x.shape) == (R, CH, T) and x.dtype == torch.float32 and x.device == w.device and x.is_contiguous()
    assert torch.equal(w.cpu(), torch.from_numpy(wave))                       # the input is unchanged
    assert not bool(x[:, BINS, :].any()) and not bool(x[:, CH - 1, :].any())  # Im of bins 0 and 2048: exactly zero
    hold("critic_spectrum R=%d n=%d T=%d %s" % (R, n, T, signal), x.cpu().numpy(), ref32, ref64, per="frame")


# ------------------------------------------------------------------------------------------------ 2. scale
def test_scale_is_applied_before_the_window():
    R, n = 3, 37 * 1024 + 11
    wave = waveform(R, n, seed=71)
    w = torch.from_numpy(wave).to(DEV)
    scaled = wave * np.float32(0.37)                                          # the float32 product torch.stft(w * scale) starts from
    assert torch.equal((w * 0.37).cpu(), torch.from_numpy(scaled))
    x = spectrum(w, 0.37)
    assert torch.equal(x, spectrum(w * 0.37, 1.0))
    hold("critic_spectrum, scale 0.37", x.cpu().numpy(), cs.ref_spectrum(scaled, torch.float32), cs.ref_spectrum(scaled, torch.float64),
         per="frame")


# ------------------------------------------------------------------------------------------------ 3. bit relations
def test_a_frame_has_the_same_bits_in_every_launch():
    """The frames of a clip's head that read no sample past the head (t * 1024 + 2047 < n1) equal the same frames of the whole clip.
    Four rows take 1024 frames per slab: the whole clip (T = 1031) runs in two slabs with frames 1024 .. 1027 in one workgroup; the heads
    run in one slab with tail chunks of two (T 6) and two (T 38) frames, and in two slabs with a tail chunk of three (T 1027)."""
    from speechseparation_amd.discriminator import spectrum_layout
    T = 1031
    w = torch.from_numpy(waveform(4, (T - 1) * HOP + 300, seed=31)).to(DEV)
    assert spectrum_layout(4, w.shape[1])["slabs"] == 2
    x = spectrum(w)
    assert x.shape[2] == T
    for T1, slabs in ((6, 1), (38, 1), (1027, 2)):
        n1 = (T1 - 1) * HOP + 100
        t = (n1 - 2048) // HOP + 1                                            # frames with t * 1024 + 2047 < n1
        assert t == T1 - 2 and (t - 1) * HOP + 2047 < n1 <= t * HOP + 2047 and spectrum_layout(4, n1)["slabs"] == slabs
        head = spectrum(w[:, :n1].contiguous())
        assert head.shape[2] == T1
        assert torch.equal(head[:, :, :t], x[:, :, :t]), T1
        del head


def test_a_row_has_the_same_bits_alone_and_in_a_batch():
    """Rows 0, 41 and 79 of the 80-row case (32 frames per slab) and rows 0, 127 and 128 of the 129-row case (two row blocks) against the
    same rows run alone (4096 frames per slab)."""
    for (R, n), rows in (((80, 20 * 1024 + 500), (0, 41, 79)), ((129, 2 * 1024 + 700), (0, 127, 128))):
        assert (R, n) in cs.CASES
        w = torch.from_numpy(waveform(R, n)).to(DEV)
        x = spectrum(w)
        for r in rows:
            assert torch.equal(spectrum(w[r:r + 1].contiguous()), x[r:r + 1]), (R, r)


def test_two_calls_give_the_same_bits():
    w = torch.from_numpy(waveform(5, 70 * 1024 + 3, seed=5)).to(DEV)
    assert torch.equal(spectrum(w, 0.6), spectrum(w, 0.6))


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_argument_errors():
    from speechseparation_amd import _native as native, spec, train
    lib, ctx = native.lib, train._context(torch.device(DEV))
    EARG, ESTATE = 1, 2                                                        # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
    w = torch.from_numpy(waveform(3, 5000, seed=9)).to(DEV)
    x = torch.full((3, CH, 5), float("nan"), device=DEV)
    before = x.clone()
    pw, px, null = ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p()
    call = lib.bsrnn_critic_spectrum

    def refused(rc, code, *words):
        msg = lib.bsrnn_last_error().decode()
        assert rc == code and all(v in msg for v in words), (rc, msg)

    refused(call(null, pw, 5000, px, 3, 4096, 1.0, None), EARG, "null context")
    refused(call(ctx, null, 5000, px, 3, 4096, 1.0, None), EARG, "null argument")
    refused(call(ctx, pw, 5000, null, 3, 4096, 1.0, None), EARG, "null argument")
    refused(call(ctx, pw, 5000, px, 0, 4096, 1.0, None), EARG, "R = 0")
    refused(call(ctx, pw, 5000, px, 3, 2048, 1.0, None), EARG, "n > 2048", "n = 2048")
    refused(call(ctx, pw, 4095, px, 3, 4096, 1.0, None), EARG, "wave_stride 4095", "n = 4096")
    refused(call(ctx, pw, 5000, px, 3, 4096, float("inf"), None), EARG, "scale = inf", "finite")
    refused(call(ctx, pw, 5000, px, 3, 4096, float("nan"), None), EARG, "scale = nan", "finite")
    refused(call(ctx, pw, 5000, px, 174678, 2049, 1.0, None), EARG, "R = 174678", "2^31")
    out = (ctypes.c_int64 * 4)()
    refused(lib.bsrnn_critic_spectrum_layout(3, 2048, out), EARG, "n = 2048")
    refused(lib.bsrnn_critic_spectrum_layout(3, 4096, None), EARG, "layout")
    v = spec.generate_bandsplits()[0]
    host = ctypes.c_void_p()
    native.check(lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(host)))
    try:
        refused(call(host, pw, 5000, px, 3, 2048, 1.0, None), EARG, "n = 2048")                # sizes before the device
        refused(call(host, pw, 5000, px, 3, 4096, 1.0, None), ESTATE, "host-only")
    finally:
        lib.bsrnn_destroy(host)
    torch.cuda.synchronize()
    assert torch.equal(x.view(torch.int32), before.view(torch.int32))          # nothing was launched
    # and the stride is honoured: rows 5000 apart, 4096 samples each
    native.check(call(ctx, pw, 5000, px, 3, 4096, 1.0, None))
    assert torch.equal(x, spectrum(w[:, :4096].contiguous()))
    with pytest.raises(native.NativeError, match="n = 2048"):
        spectrum(w[:, :2048].contiguous())


# ------------------------------------------------------------------------------------------------ 5. the entry point
def _rel(a, ref):
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def test_train_discriminator_entry_point_at_4096(tmp_path):
    """train-discriminator.py --n_fft 4096 trains the reference's default critic; its discriminator.pth loads into the stock 4098-channel
    module, and with those weights the device's score of one synthetic clip (critic_spectrum, then Discriminator()) is held to the stock
    modules' own float32 error against float64: max|a - ref64| / max|ref64| at most 4 x stock fp32's plus one fp32 ulp (2^-23), the rule
    tests/test_gpu_critic.py applies to the module."""
    from speechseparation_amd import weights
    from speechseparation_amd.discriminator import Discriminator
    script = os.path.join(REPO, "train-discriminator.py")
    out = subprocess.run([sys.executable, script, "--n_fft", "4096", "--synthetic", "2", "--mini", "--epochs", "1"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "4096-point" in out.stdout and "Epoch 0 Loss" in out.stdout and "Validation Loss" in out.stdout
    sd = torch.load(str(tmp_path / "discriminator.pth"), map_location="cpu", weights_only=True)
    ref64, ref32 = cr.CriticF64(4098), cr.CriticF64(4098, dtype=torch.float32)
    ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ref32.load_state_dict(sd, strict=True)
    D = Discriminator()
    D.load_state_dict(sd, strict=True)
    D = D.to(DEV)
    wave = weights.synth_waveform(2, 600 * 1024, seed=3000)
    with torch.no_grad():
        s = D(spectrum(torch.from_numpy(wave).to(DEV))).cpu()
        s64 = ref64(torch.from_numpy(cs.ref_spectrum(wave, torch.float64)))
        s32 = ref32(torch.from_numpy(cs.ref_spectrum(wave, torch.float32)))
    e_dev, e_cpu = _rel(s, s64), _rel(s32, s64)
    print("score: device %.3e   stock fp32 %.3e" % (e_dev, e_cpu))
    assert tuple(s.shape) == (1,) and e_dev <= 4 * e_cpu + 2.0 ** -23, (e_dev, e_cpu)
