"""GPU: ragged training - the clips of one optimizer step as one padded batch R x Tmax with one backward pass (include/bsrnn_hip.h, "ragged
training"; speechseparation_amd/train.py: stft_ragged, IstftRaggedFunction, TriLossRaggedFunction, train_loss_ragged, train_backward_many,
train_step_many; train.py --ragged).  The DSP ends against the rectangular calls on each clip alone (bit for bit) and torch.istft's autograd
transpose in float64, the per-clip loss and its gradients against torch on the CPU, the whole model against the float64 restatement clip by
clip, and the step against the clip-by-clip accumulation it replaces."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [5 * 1024 + 300, 3 * 1024 + 77, 1025, 6 * 1024]      # T = 6, 4, 2, 7
STRIDE = 6 * 1024 + 3                                       # every other row is off 16-byte alignment
NAN = float("nan")


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(1e-30, float(b.abs().max())))


def _frames(n):
    return 1 + n // 1024


def _i64(v):
    return (ctypes.c_int64 * len(v))(*v)


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


def _ragged_waves(lens, stride, seed):
    """[R, stride] on the GPU: row r holds lens[r] random samples, NaN behind them."""
    g = torch.Generator().manual_seed(seed)
    w = torch.full((len(lens), stride), NAN)
    for r, n in enumerate(lens):
        w[r, :n] = torch.randn(n, generator=g)
    return w.cuda()


# ------------------------------------------------------------------------------------------------ 1. the DSP ends alone
def test_stft_ragged_is_stft_of_each_clip_and_zeros_behind_it():
    from speechseparation_amd import train
    wave = _ragged_waves(LENS, STRIDE, 1)
    T = max(_frames(n) for n in LENS)
    dev = wave.device
    x = torch.full((4, 2050, T), NAN, device=dev)
    train._native.check(train._lib.bsrnn_stft_ragged(train._context(dev), train._p(wave), STRIDE, _i64(LENS), train._p(x), 4, train._s(dev)))
    assert torch.equal(x, train.stft_ragged(wave, LENS))
    for r, n in enumerate(LENS):
        alone = train.stft(wave[r:r + 1, :n].contiguous())
        assert tuple(alone.shape) == (1, 2050, _frames(n))
        assert torch.equal(x[r:r + 1, :, :_frames(n)], alone), r                    # bit-identical: the shared walk
        assert float(x[r, :, _frames(n):].abs().sum()) == 0.0 and not torch.isnan(x[r]).any(), r


def test_istft_ragged_and_its_transpose_row_by_row():
    from speechseparation_amd import train
    torch.manual_seed(2)
    T = max(_frames(n) for n in LENS)
    y = torch.randn(4, 2050, T)
    dwave = torch.randn(4, (T - 1) * 1024)
    for r, n in enumerate(LENS):
        y[r, :, _frames(n):] = NAN                                                   # frames behind a row's end are not used ...
        dwave[r, (_frames(n) - 1) * 1024:] = NAN                                     # ... and gradient behind its samples is never read
    yg = y.cuda().requires_grad_(True)
    out = train.IstftRaggedFunction.apply(yg, LENS)
    assert tuple(out.shape) == (4, (T - 1) * 1024) and not torch.isnan(out).any()
    out.backward(dwave.cuda())
    out, dy = out.detach(), yg.grad
    assert tuple(dy.shape) == (4, 2050, T) and not torch.isnan(dy).any()
    worst_alone = worst_torch = 0.0
    for r, n in enumerate(LENS):
        Tr, n_est = _frames(n), (_frames(n) - 1) * 1024
        yr = y[r:r + 1, :, :Tr].contiguous().cuda().requires_grad_(True)
        alone = train.IstftFunction.apply(yr)
        assert torch.equal(out[r:r + 1, :n_est], alone.detach()), r                  # forward: bit-identical per row
        assert float(out[r, n_est:].abs().sum()) == 0.0, r                           # zeros follow the real samples
        alone.backward(dwave[r:r + 1, :n_est].contiguous().cuda())
        e = _rel(dy[r:r + 1, :, :Tr], yr.grad)
        worst_alone = max(worst_alone, e)
        assert e < 1e-6, (r, e)
        assert torch.equal(dy[r:r + 1, :, :Tr], yr.grad), r                          # the three passes of bsrnn_istft_backward were kept: the same bits
        assert float(dy[r, :, Tr:].abs().sum()) == 0.0, r                            # exact zeros in the padded frames ...
        assert float(dy[r, 1, :].abs().max()) == 0.0 and float(dy[r, 2049, :].abs().max()) == 0.0, r      # ... and in Im of bins 0 and 1024
        # the autograd transpose of torch.istft in float64 on the CPU
        yd = y[r:r + 1, :, :Tr].double().requires_grad_(True)
        yc = yd.reshape(1, 1025, 2, Tr)
        w = torch.istft(torch.complex(yc[:, :, 0, :], yc[:, :, 1, :]), n_fft=2048, hop_length=1024, window=torch.hann_window(2048, dtype=torch.float64))
        (w * dwave[r:r + 1, :n_est].double()).sum().backward()
        e = _rel(dy[r:r + 1, :, :Tr], yd.grad)
        worst_torch = max(worst_torch, e)
        assert e < 1e-5, (r, e)
    print("ragged iSTFT backward: %.1e from bsrnn_istft_backward per clip, %.1e from torch.istft's transpose in float64" % (worst_alone, worst_torch))


def _fresh_context(train, dev):
    v = train.generate_bandsplits()[0]
    ctx = ctypes.c_void_p()
    train._native.check(train._lib.bsrnn_create(dev.index, _i32(v), len(v), ctypes.byref(ctx)))
    return ctx


def test_queued_ragged_calls_pass_the_eighth_upload_mirror_and_a_growth():
    """The lengths of a ragged call travel through eight pinned mirrors used in turn and one device block that grows (api_internal.h,
    UploadRing).  Twenty bsrnn_stft_ragged calls of 1 to 6 rows and 1025 to 5 * 1024 samples, other lengths in every call, queue up on a side
    stream with no host synchronisation between them: each mirror is written three times.  The block is allocated in units of 256 bytes, so
    the lengths of up to 32 rows never outgrow the first one; two more calls, of 40 and of 72 rows, stand behind the tenth and the
    seventeenth and make it grow twice after the eighth call.  One synchronisation, then every output bit for bit against the same call
    made alone on a context of its own."""
    from speechseparation_amd import train
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 40, 5, 6, 6, 1, 3, 6, 2, 72, 6, 4, 6]
    stride = 5 * 1024 + 3
    rng = np.random.RandomState(7)
    calls = []
    for i, R in enumerate(rows):
        lens = [int(n) for n in rng.randint(1025, 5 * 1024 + 1, size=R)]
        T = max(_frames(n) for n in lens)
        calls.append((lens, _ragged_waves(lens, stride, 100 + i), torch.full((R, 2050, T), NAN, device=dev), torch.full((R, 2050, T), NAN, device=dev)))
    assert len({tuple(c[0]) for c in calls}) == len(calls)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    ctx = _fresh_context(train, dev)
    try:
        for lens, wave, x, _ in calls:
            train._native.check(train._lib.bsrnn_stft_ragged(ctx, train._p(wave), stride, _i64(lens), train._p(x), len(lens),
                                                             ctypes.c_void_p(side.cuda_stream)))
        side.synchronize()
    finally:
        train._lib.bsrnn_destroy(ctx)
    for i, (lens, wave, x, alone) in enumerate(calls):
        ctx = _fresh_context(train, dev)
        try:
            train._native.check(train._lib.bsrnn_stft_ragged(ctx, train._p(wave), stride, _i64(lens), train._p(alone), len(lens),
                                                             ctypes.c_void_p(side.cuda_stream)))
            side.synchronize()
        finally:
            train._lib.bsrnn_destroy(ctx)
        assert not torch.isnan(alone).any() and torch.equal(x, alone), (i, lens)


# ------------------------------------------------------------------------------------------------ 2. the loss alone
def _loss_native(train, y, s, xt, sp, lens, rows):
    dev = y.device
    values = torch.full((len(lens), 5), NAN, device=dev, dtype=torch.float64)
    sums = torch.full((y.shape[0], 2), NAN, device=dev, dtype=torch.float64)
    train._native.check(train._lib.bsrnn_train_loss_ragged(train._context(dev), train._p(y), train._p(s), train._p(xt), train._p(sp), sp.shape[1],
                                                           _i64(lens), _i32(rows), len(lens), train._p(values), train._p(sums), train._s(dev)))
    return values, sums


def _loss_backward_native(train, y, s, xt, sp, lens, rows, sums, gclip):
    dev = y.device
    dy, dx = torch.full_like(y, NAN), torch.full_like(xt, NAN)
    train._native.check(train._lib.bsrnn_train_loss_ragged_backward(train._context(dev), train._p(y), train._p(s), train._p(xt), train._p(sp), sp.shape[1],
                                                                    _i64(lens), _i32(rows), len(lens), train._p(sums), train._p(gclip), train._p(dy),
                                                                    train._p(dx), train._s(dev)))
    return dy, dx


# clips of [2, 1, 1] rows, rows 0-1 share a length.  Tmax = 7 with an odd stride: scalar loads in the time kernels, and spans of the spectral
# kernels that start off a 16-byte boundary in every other row; Tmax = 7 / 6 with a stride that is a multiple of 4: the 16-byte loads, with
# and without a scalar head; the clip of 1 025 samples has two frames and one hop.
@pytest.mark.parametrize("clip_lens,stride", [([LENS[0], LENS[1], LENS[3]], STRIDE), ([LENS[0], LENS[2], LENS[3]], STRIDE + 1),
                                              ([LENS[0], LENS[1], LENS[2]], STRIDE + 1)])
def test_tri_loss_ragged_values_and_gradients_per_clip(clip_lens, stride):
    from speechseparation_amd import train
    rows = [2, 1, 1]
    row_lens = [n for n, ch in zip(clip_lens, rows) for _ in range(ch)]
    R, T = 4, max(_frames(n) for n in clip_lens)
    g = torch.Generator().manual_seed(7)
    y, s = torch.randn((R, 2050, T), generator=g), torch.randn((R, 2050, T), generator=g)
    xt, sp = torch.randn((R, (T - 1) * 1024), generator=g), torch.randn((R, stride), generator=g)
    y[0, 5, 1] = s[0, 5, 1]                                                          # a zero difference: sgn(0) = 0
    xt[1, 17] = sp[1, 17]
    for r, n in enumerate(row_lens):                                                 # NaN in every padded position
        y[r, :, _frames(n):] = NAN
        s[r, :, _frames(n):] = NAN
        xt[r, (_frames(n) - 1) * 1024:] = NAN
        sp[r, n:] = NAN
    gclip = torch.tensor([[0.7, -1.3], [-0.4, 0.9], [1.1, 0.6]])

    # torch on the CPU, per clip: the differences formed in fp32, then float64 arithmetic
    want = torch.zeros((3, 5), dtype=torch.float64)
    want_sums = torch.zeros((R, 2), dtype=torch.float64)
    want_dy, want_dx = torch.zeros_like(y, dtype=torch.float64), torch.zeros_like(xt, dtype=torch.float64)
    r0 = 0
    for c, (n, ch) in enumerate(zip(clip_lens, rows)):
        Tc, n_est = _frames(n), (_frames(n) - 1) * 1024
        d = (y[r0:r0 + ch, :, :Tc] - s[r0:r0 + ch, :, :Tc]).double().requires_grad_(True)
        dt = (xt[r0:r0 + ch, :n_est] - sp[r0:r0 + ch, :n_est]).double().requires_grad_(True)
        l1_t, l1_re, l1_im = dt.abs().mean(), d[:, 0::2].abs().mean(), d[:, 1::2].abs().mean()
        ss, dd = sp[r0:r0 + ch, :n_est].double().square().sum(1), dt.square().sum(1)
        sdr = (10 * torch.log10((ss + 1e-9) / (dd + 1e-9))).mean()
        loss = l1_t + l1_re + l1_im
        (float(gclip[c, 0]) * loss + float(gclip[c, 1]) * sdr).backward()
        want[c] = torch.stack([loss, l1_t, l1_re, l1_im, sdr]).detach()
        want_sums[r0:r0 + ch, 0], want_sums[r0:r0 + ch, 1] = ss, dd.detach()
        want_dy[r0:r0 + ch, :, :Tc], want_dx[r0:r0 + ch, :n_est] = d.grad, dt.grad
        r0 += ch

    yd, sd, xd, pd = y.cuda(), s.cuda(), xt.cuda(), sp.cuda()
    values, sums = _loss_native(train, yd, sd, xd, pd, clip_lens, rows)
    dy, dx = _loss_backward_native(train, yd, sd, xd, pd, clip_lens, rows, sums, gclip.cuda())
    e_val = float(((values.cpu() - want).abs() / want.abs()).max())
    e_sum = float(((sums.cpu() - want_sums).abs() / want_sums.abs()).max())
    e_dy, e_dx = _rel(dy, want_dy), _rel(dx, want_dx)
    print("ragged tri-loss, Tmax %d stride %d: values %.1e, row sums %.1e (relative); dy %.1e, dxtime %.1e of the largest element" % (
        T, stride, e_val, e_sum, e_dy, e_dx))
    assert e_val < 1e-9 and e_sum < 1e-9                    # only the order of the double additions differs
    assert e_dy < 1e-6 and e_dx < 1e-6                      # a sign times one fp32 weight / a handful of fp32 operations
    assert not torch.isnan(dy).any() and not torch.isnan(dx).any() and not torch.isnan(values).any() and not torch.isnan(sums).any()
    for r, n in enumerate(row_lens):                        # exact zeros at every padded position
        assert float(dy[r, :, _frames(n):].abs().sum()) == 0.0 and float(dx[r, (_frames(n) - 1) * 1024:].abs().sum()) == 0.0, r
    assert float(dy[0, 5, 1]) == 0.0
    # a second run is bit-identical
    values2, sums2 = _loss_native(train, yd, sd, xd, pd, clip_lens, rows)
    dy2, dx2 = _loss_backward_native(train, yd, sd, xd, pd, clip_lens, rows, sums2, gclip.cuda())
    assert torch.equal(values, values2) and torch.equal(sums, sums2) and torch.equal(dy, dy2) and torch.equal(dx, dx2)
    # the autograd function is these two calls
    yg, xg = yd.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    losses, sdrs = train.TriLossRaggedFunction.apply(yg, sd, xg, pd, clip_lens, rows)
    assert losses.dtype == torch.float32 and torch.equal(losses, values[:, 0].float()) and torch.equal(sdrs, values[:, 4].float())
    (losses * gclip[:, 0].cuda() + sdrs * gclip[:, 1].cuda()).sum().backward()
    assert torch.equal(yg.grad, dy) and torch.equal(xg.grad, dx)


# ------------------------------------------------------------------------------------------------ 3. the whole model
CLIPS = [5420, 3149, 1025]                                  # 6, 4 and 2 frames


def _clip(c):
    from speechseparation_amd import weights
    return (torch.from_numpy(weights.synth_waveform(2, CLIPS[c], seed=20 + c)), torch.from_numpy(weights.synth_waveform(2, CLIPS[c], seed=40 + c)))


def _model(sd):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().train()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd.items()})
    return m.to("cuda:0")


def _cpu_clip_by_clip(sd, dtype):
    """The reference's accumulation on the CPU restatement of the model: per-clip loss and SDR, and the gradients of their sums."""
    from oracle.bsrnn_torch_cpu import TorchCpuBSRNN
    from speechseparation_amd import spec
    ref = TorchCpuBSRNN(sd, spec.generate_bandsplits()[0], dtype=dtype)
    params = ref.trainable()
    names = [k for k in params if params[k].numel() > 0]
    win = torch.hann_window(2048, dtype=dtype)
    losses, sdrs = [], []
    g_loss, g_sdr = {k: torch.zeros_like(params[k]) for k in names}, {k: torch.zeros_like(params[k]) for k in names}
    for c in range(len(CLIPS)):
        mix, speech = (t.to(dtype) for t in _clip(c))
        X = torch.stft(mix, n_fft=2048, hop_length=1024, return_complex=True, window=win)
        y = ref.forward_differentiable(torch.stack((X.real, X.imag), dim=2).reshape(2, 2050, -1))
        yc = y.reshape(2, -1, 2, y.shape[2])
        Y = torch.complex(yc[:, :, 0, :], yc[:, :, 1, :])
        xt = torch.istft(Y, n_fft=2048, hop_length=1024, window=win)
        S = torch.stft(speech, n_fft=2048, hop_length=1024, return_complex=True, window=win)
        st = speech[:, :xt.shape[1]]
        l1 = torch.nn.L1Loss(reduction="mean")
        loss = l1(xt, st) + l1(Y.real, S.real) + l1(Y.imag, S.imag)
        sdr = (10 * torch.log10((st.square().sum(1) + 1e-9) / ((xt - st).square().sum(1) + 1e-9))).mean()
        for acc, obj in ((g_loss, loss), (g_sdr, -sdr)):
            for k, g in zip(names, torch.autograd.grad(obj, [params[k] for k in names], retain_graph=True, allow_unused=True)):
                if g is not None:
                    acc[k] += g
        losses.append(float(loss.detach()))
        sdrs.append(float(sdr.detach()))
    return losses, sdrs, g_loss, g_sdr


@pytest.fixture(scope="module")
def oracle64():
    from speechseparation_amd import weights
    sd = weights.synth_state_dict(None, seed=0)
    return sd, _cpu_clip_by_clip(sd, torch.float64)


def _worst(grads, ref):
    worst = ("", 0.0)
    for k, g_ref in ref.items():
        e = _rel(grads[k], g_ref) if float(g_ref.abs().max()) > 0 else float(grads[k].abs().max())
        worst = max(worst, (k, e), key=lambda t: t[1])
    return worst


def _packed():
    mix, speech = torch.zeros((6, max(CLIPS))), torch.zeros((6, max(CLIPS)))
    for c, n in enumerate(CLIPS):
        mix[2 * c:2 * c + 2, :n], speech[2 * c:2 * c + 2, :n] = _clip(c)
    return mix.cuda(), speech.cuda()


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.numel() > 0}


def test_padded_batch_gradient_is_the_sum_of_the_clips_gradients(oracle64):
    from speechseparation_amd import train
    sd, (ref_losses, ref_sdrs, ref_g_loss, ref_g_sdr) = oracle64
    m = _model(sd)
    mix, speech = _packed()
    lens, rows = CLIPS, [2, 2, 2]
    losses, sdrs, x_time = train.train_loss_ragged(m, mix, speech, lens, rows)
    assert tuple(losses.shape) == tuple(sdrs.shape) == (3,) and losses.dtype == sdrs.dtype == torch.float32 and losses.requires_grad and sdrs.requires_grad
    assert tuple(x_time.shape) == (6, 5 * 1024)
    for c in range(3):
        print("clip %d: loss %.7f (float64 %.7f), sdr %.5f (float64 %.5f)" % (c, float(losses[c]), ref_losses[c], float(sdrs[c]), ref_sdrs[c]))
        assert abs(float(losses[c]) - ref_losses[c]) < 1e-5 * abs(ref_losses[c])
        assert abs(float(sdrs[c]) - ref_sdrs[c]) < 1e-4 * max(1.0, abs(ref_sdrs[c]))
    losses.sum().backward()
    g_loss = _grads(m)
    w_loss = _worst(g_loss, ref_g_loss)
    for p in m.parameters():
        p.grad = None
    losses2, sdrs2, _ = train.train_loss_ragged(m, mix, speech, lens, rows)
    (-sdrs2.sum()).backward()
    g_sdr = _grads(m)
    w_sdr = _worst(g_sdr, ref_g_sdr)
    # the fp32 CPU restatement of the same sum against the same float64 oracle: what fp32 arithmetic alone costs
    _, _, cpu32_g_loss, _ = _cpu_clip_by_clip(sd, torch.float32)
    w_cpu32 = _worst(cpu32_g_loss, ref_g_loss)
    print("worst per-tensor gradient error against float64: loss %.2e (%s), -sdr %.2e (%s); the fp32 CPU restatement %.2e (%s)" % (
        w_loss[1], w_loss[0], w_sdr[1], w_sdr[0], w_cpu32[1], w_cpu32[0]))
    # ... and the clip-by-clip accumulation on the GPU through train_loss
    for p in m.parameters():
        p.grad = None
    for c in range(3):
        mx, sp = (t.cuda() for t in _clip(c))
        loss, xt = train.train_loss(m, mx, sp)
        loss.backward()
        assert abs(float(loss) - float(losses[c])) < 1e-5 * abs(float(loss))
    w_acc = _worst(g_loss, _grads(m))
    w_acc64 = _worst(_grads(m), ref_g_loss)                  # (gradients accumulated over several backward passes: b_ih and b_hh must not share a tensor)
    print("against the clip-by-clip accumulation on the GPU: %.2e (%s); that accumulation against float64: %.2e (%s)" % (
        w_acc[1], w_acc[0], w_acc64[1], w_acc64[0]))
    assert w_acc64[1] < 1e-3, w_acc64
    assert len(g_loss) >= 280 and w_loss[1] < 1e-3 and w_sdr[1] < 1e-3, (w_loss, w_sdr)
    assert w_acc[1] < 1e-3, w_acc


# ------------------------------------------------------------------------------------------------ 4. one clip is train_loss
def test_one_clip_at_its_own_length_is_train_loss(oracle64):
    from speechseparation_amd import train
    sd = oracle64[0]
    m = _model(sd)
    mix, speech = (t.cuda() for t in _clip(0))
    n = CLIPS[0]
    loss, x_time = train.train_loss(m, mix, speech)
    loss.backward()
    want = _grads(m)
    for p in m.parameters():
        p.grad = None
    losses, sdrs, x_time_r = train.train_loss_ragged(m, mix, speech, [n], [2])
    losses.sum().backward()
    assert abs(float(losses[0]) - float(loss)) < 1e-6 * abs(float(loss))
    assert abs(float(sdrs[0]) - float(train.sdr(x_time, speech[:, :x_time.shape[1]]))) < 1e-4
    w = _worst(_grads(m), want)
    print("one clip: loss %.8f against %.8f, worst gradient difference %.2e (%s)" % (float(losses[0]), float(loss), w[1], w[0]))
    assert w[1] < 1e-5, w
    # the STFT and the iSTFT inside it share the walks of the rectangular calls: the same bits
    x = train.stft(mix)
    assert torch.equal(train.stft_ragged(mix, [n, n]), x)
    y = train.forward_train(m, x).detach()
    assert torch.equal(train.IstftRaggedFunction.apply(y, [n, n]), train.IstftFunction.apply(y))


# ------------------------------------------------------------------------------------------------ 5. buckets and the step
PAIR_LENS = [5420, 3149, 1025, 4500, 2100]


def _pairs():
    from speechseparation_amd import weights
    return [(torch.from_numpy(weights.synth_waveform(2, n, seed=60 + i)).cuda(), torch.from_numpy(weights.synth_waveform(2, n, seed=80 + i)).cuda())
            for i, n in enumerate(PAIR_LENS)]


def test_buckets_accumulate_and_the_step_follows_the_clip_by_clip_step(oracle64):
    from speechseparation_amd import _native, spec, train
    sd = oracle64[0]
    pairs = _pairs()
    assert len(spec.ragged_buckets([_frames(n) for n in PAIR_LENS], [2] * 5, 4, 0.25)) >= 2
    a, b = _model(sd), _model(sd)
    got = train.train_backward_many(a, pairs, max_rows=4)
    want = []
    for mix, speech in pairs:
        loss, xt = train.train_loss(b, mix, speech)
        loss.backward()
        want.append((float(loss), float(train.sdr(xt, speech[:, :xt.shape[1]]))))
    assert len(got) == 5 and all(isinstance(v, float) for t in got for v in t)
    for (l, s), (lw, sw) in zip(got, want):
        assert abs(l - lw) < 1e-5 * abs(lw) and abs(s - sw) < 1e-4 * max(1.0, abs(sw)), (got, want)
    w = _worst(_grads(a), _grads(b))
    print("five pairs in buckets of at most 4 rows: worst gradient difference to the clip-by-clip accumulation %.2e (%s)" % (w[1], w[0]))
    assert w[1] < 1e-3, w

    # two optimizer steps each way, from the same weights
    a, b = _model(sd), _model(sd)
    opt_a, opt_b = train.AdamW(a.parameters(), lr=1e-3, weight_decay=1e-2), train.AdamW(b.parameters(), lr=1e-3, weight_decay=1e-2)
    first = train.train_step_many(a, opt_a, pairs, max_rows=4)
    allocs = _native.lib.bsrnn_debug_counter(0)
    second = train.train_step_many(a, opt_a, pairs, max_rows=4)
    assert _native.lib.bsrnn_debug_counter(0) == allocs              # the same shapes again: no first-use work
    assert all(p.grad is None for p in a.parameters())
    ref = []
    for _ in range(2):
        step = []
        for mix, speech in pairs:
            loss, _ = train.train_loss(b, mix, speech)
            loss.backward()
            step.append(float(loss))
        opt_b.step()
        opt_b.zero_grad()
        ref.append(step)
    print("second step, per-clip losses", [l for l, _ in second], "clip by clip", ref[1])
    assert sum(l for l, _ in second) < sum(l for l, _ in first)
    for (l, _), lw in zip(second, ref[1]):
        assert abs(l - lw) < 2e-4 * abs(lw), (second, ref[1])


# ------------------------------------------------------------------------------------------------ 6. the entry point
def test_train_entry_point_with_ragged_prints_the_same_epochs(tmp_path):
    import subprocess
    import sys
    from conftest import REPO
    from speechseparation_amd import audio, weights
    data = tmp_path / "data"
    for split, count, seed0 in (("train", 5, 300), ("val", 2, 400)):
        for i in range(count):
            d = data / split / ("clip%d" % i)
            d.mkdir(parents=True)
            n = 16000 + (i * 3989 + 1234) % 16000                       # 1 - 2 s at 16 kHz, all different
            audio.save_wav(str(d / "mixture.wav"), torch.from_numpy(weights.synth_waveform(2, n, seed=seed0 + 2 * i)), 16000)
            audio.save_wav(str(d / "speech.wav"), torch.from_numpy(weights.synth_waveform(2, n, seed=seed0 + 2 * i + 1)), 16000)
    env = dict(os.environ, PYTHONPATH=REPO)
    runs = {}
    for tag, extra in (("clips", []), ("ragged", ["--ragged"])):
        out = tmp_path / tag
        out.mkdir()
        cmd = [sys.executable, os.path.join(REPO, "train.py"), "--datapath", str(data), "--batch_size", "3", "--epochs", "2",
               "--synthetic-weights", "0", "--outdir", str(out)] + extra
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        ep = [(float(l.split()[3]), float(l.split()[5])) for l in p.stdout.splitlines() if l.startswith("Epoch") and "Loss" in l]
        va = [(float(l.split()[2]), float(l.split()[5])) for l in p.stdout.splitlines() if l.startswith("Validation Loss")]
        runs[tag] = (ep, va)
        print(tag, ep, va)
        for f in ("model.pth", "model-always.pth", "optimizer.pth", "optimizer-always.pth"):
            assert (out / f).exists(), (tag, f)
    (c_ep, c_va), (r_ep, r_va) = runs["clips"], runs["ragged"]
    assert len(r_ep) == 2 and len(r_va) == 2 and len(c_ep) == 2 and len(c_va) == 2
    for a, b in zip(r_ep + r_va, c_ep + c_va):
        assert abs(a[0] - b[0]) <= 1e-5 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-4 * max(1.0, abs(b[1])), (runs["ragged"], runs["clips"])
    assert math.isfinite(r_ep[1][0]) and r_ep[1][0] < r_ep[0][0]
