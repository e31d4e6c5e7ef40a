"""The training kernels (csrc/lstm_train.hip, csrc/train_ops.hip) at the shapes of a real training step, against float64.

Every comparison has three legs: a float64 reference on the CPU (torch autograd in float64 for the LSTM, Linear and whole-model
cases; a float64 restatement of torch.optim.AdamW for the optimizer), the same operation in fp32 CPU torch (its error against
float64 is e_f32) and the library (e_gpu).  Errors are max-abs differences normalised by the float64 tensor's max-abs, and the
bound is e_gpu <= 3 e_f32 + FLOOR, as in test_gpu_exact_path.py.  Weight gradients are also checked row by row (each output
unit's row normalised by that row's own max-abs, bound 3 e_f32(row) + FLOOR): a wrong chunk or tile that touches only a few
small rows shows there.  FLOOR = 2e-6.  Dropping one of the at most 256 row chunks of a weight-gradient reduction changes a
gradient by about 1/chunks relative or more (>= 4e-3), three orders of magnitude above FLOOR.

The weight-gradient reductions run in row chunks (train_ops.hip: chunk_count / rows_per_chunk).  The layout of every case comes
from the library's own query, train.reduction_layout (bsrnn_train_reduction_layout), and test_shapes_reach_every_reduction_layout
asserts from it that the cases reach each regime of the chunk count - about M / 512, the LSTM_TRAIN_CHUNKS cap of 64, the fill
count ceil(1024 / tiles), the cap ceil(M / 64), the LSTM_TRAIN_MAX_CHUNKS clamp of 256 -, a single chunk, every chunk count mod 4
(reduce_partials_kernel sums four chunks at a time, then a remainder) and chunks of 16 mod 32 rows (the partial kernel walks 32-row
slabs, so such a chunk ends in a half slab).  An LSTM gradient has at most 8 tiles, so its fill count (>= 128) always exceeds the
cap of 64: the M / 512 and cap regimes are reached by Linear shapes.

LeakyReLU's derivative jumps at 0.  Where a float64 pre-activation lies within rounding reach of 0 (|p| < 1e-5 max |p|) the
upstream gradient is set to 0, so that no leg can pick the other branch by rounding; pre-activations that are exactly 0 in every
leg (zero input rows, zero bias) keep theirs: there torch's slope is 0.01, and the library must agree.  The whole-model case
cannot mask inside the model; it prints how close its float64 pre-activations and L1 terms come to their kinks.

AdamW is compared after 1, 2 and 50 steps with double betas, as torch holds them (1 - 0.999f is 1.3e-5 off 1 - 0.999).
"""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
F64 = torch.float64
LSTM_TRAIN_CHUNKS, LSTM_TRAIN_MAX_CHUNKS = 64, 256       # csrc/kernels.h
GEMM_GROUP, ADAM_GROUP = 12, 80                           # csrc/kernels.h: jobs per grouped GEMM / AdamW launch


def _err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    d = float((got - ref).abs().max()) if ref.numel() else 0.0
    return d / scale if scale > 0 else d


def _row_err(got, ref):
    """Per row of a weight gradient [rows, cols]: max |got - ref| / max |ref| of that row (absolute where the row is all 0)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d, s = (got - ref).abs().amax(1), ref.abs().amax(1)
    return torch.where(s > 0, d / torch.where(s > 0, s, torch.ones_like(s)), d)


def _check(label, layout, name, gpu, f32, f64, rows=False):
    e_gpu, e_f32 = _err(gpu, f64), _err(f32, f64)
    bound = 3 * e_f32 + FLOOR
    print("%-34s %-22s %-6s e_gpu %.2e  e_f32 %.2e  bound %.2e" % (label, layout, name, e_gpu, e_f32, bound))
    assert e_gpu <= bound, (label, name, e_gpu, e_f32)
    if rows:
        g, c = _row_err(gpu, f64), _row_err(f32, f64)
        excess = g - (3 * c + FLOOR)
        worst = int(excess.argmax())
        print("%-34s %-22s %-6s rows: worst row %d e_gpu %.2e  e_f32 %.2e" % (label, layout, name, worst, float(g[worst]), float(c[worst])))
        assert float(excess.max()) <= 0, (label, name, "row", worst, float(g[worst]), float(c[worst]))


def _fmt(layouts):
    return " ".join("%dx%d" % lay for lay in layouts)


# ------------------------------------------------------------------------------------------ 1. LSTM layer
# (N, L, IN, ndir, gain)
LSTM_CASES = [
    (8064, 12, 64, 2, 3.0),        # the bench's band-axis layer 0 (64 rows x 126 frames, 12 bands): dw_hh 252 chunks of 384 rows
    (8064, 12, 128, 2, 3.0),       # band-axis layer 1: dw_ih 126 chunks of 768 rows (the remainder path)
    (768, 126, 64, 1, 3.0),        # the bench's time-axis layer (64 rows x 12 bands, T = 126)
    (126, 12, 64, 2, 1.0),         # train.py's default clip (2 rows x 64 000 samples, T = 63): band axis
    (24, 63, 64, 1, 1.0),          # ... and time axis
    (1697, 12, 64, 2, 3.0),        # N % 16 = 1; 255 chunks (mod 4 = 3) of 80 rows (16 mod 32: a half slab ends each chunk)
    (47, 12, 128, 2, 1.0),         # N % 16 = 15
    (1, 300, 64, 1, 3.0),          # one long sequence
    (1000, 1, 64, 2, 1.0),         # L = 1: the step shift masks every h_prev read of dw_hh
    (1024, 12, 128, 2, 1.0),       # dw_ih at the fill count (128 chunks of 96 rows)
    (5, 12, 64, 2, 1.0),           # a single chunk
]


def _lstm_layouts(N, L, IN):
    from speechseparation_amd import train
    return [train.reduction_layout(N * L, 256, IN), train.reduction_layout(N * L, 256, 64)]


def _lstm_legs(lstm, x, dh):
    x = x.clone().requires_grad_(True)
    h, _ = lstm(x)
    (h * dh).sum().backward()
    return h.detach(), x.grad


@pytest.mark.parametrize("N,L,IN,ndir,gain", LSTM_CASES)
def test_lstm_layer_against_float64(N, L, IN, ndir, gain):
    from speechseparation_amd import train
    torch.manual_seed(1000 + N + L + IN)
    l32 = torch.nn.LSTM(IN, 64, batch_first=True, bidirectional=ndir == 2)
    with torch.no_grad():
        for p in l32.parameters():
            p.mul_(gain)
    l64 = copy.deepcopy(l32).to(F64)
    x = torch.randn(N, L, IN)
    dh = torch.randn(N, L, ndir * 64)
    h32, dx32 = _lstm_legs(l32, x, dh)
    h64, dx64 = _lstm_legs(l64, x.to(F64), dh.to(F64))
    sfx = ["", "_reverse"][:ndir]
    grads = lambda m, name: torch.stack([getattr(m, name + "_l0" + s).grad for s in sfx])      # noqa: E731

    w_ih, w_hh, b_ih, b_hh = [t.detach().cuda() for t in train.stack_direction_weights(l32, 0)]
    xg = x.cuda()
    h, gates, cells = train.lstm_layer_forward(xg, w_ih, w_hh, b_ih + b_hh)
    dx, dw_ih, dw_hh, db = train.lstm_layer_backward(xg, h, gates, cells, dh.cuda(), w_ih, w_hh)
    torch.cuda.synchronize()

    label = "lstm N=%d L=%d IN=%d ndir=%d g=%.0f" % (N, L, IN, ndir, gain)
    lay = _fmt(_lstm_layouts(N, L, IN))
    _check(label, lay, "h", h, h32, h64)
    _check(label, lay, "dx", dx, dx32, dx64)
    _check(label, lay, "dw_ih", dw_ih.reshape(-1, IN), grads(l32, "weight_ih").reshape(-1, IN), grads(l64, "weight_ih").reshape(-1, IN), rows=True)
    _check(label, lay, "dw_hh", dw_hh.reshape(-1, 64), grads(l32, "weight_hh").reshape(-1, 64), grads(l64, "weight_hh").reshape(-1, 64), rows=True)
    _check(label, lay, "db", db, grads(l32, "bias_ih"), grads(l64, "bias_ih"))


# ------------------------------------------------------------------------------------------ 2. Linear (+ LeakyReLU)
# (M, K, N, leaky, special)
LINEAR_CASES = [
    (8064, 768, 768, True, None),      # the 768 x 768 layers at the bench's 8 064 rows: 16 chunks of 512 rows (about M / 512)
    (8064, 2, 2, True, None),          # the first band of the default table (1 bin: 2 features)
    (8064, 514, 514, True, None),      # the last live band (257 bins)
    (8065, 64, 64, True, None),        # M % 64 = 1
    (8127, 65, 514, False, None),      # M % 64 = 63
    (1000, 1, 65, True, None),         # K = 1, N = 65
    (3000, 17, 1, True, None),         # K = 17, N = 1
    (2000, 514, 65, False, None),      # K = 514
    (16400, 1, 1, True, None),         # a 1-tile gradient past 256 x 64 rows: 205 chunks of 80 rows (half slabs)
    (20480, 17, 1, False, None),       # a 1-tile gradient at the 256-chunk clamp
    (33792, 320, 320, False, None),    # 25 tiles (fill 41) at the 64-chunk cap
    (777, 64, 64, True, "zero"),       # exactly-zero pre-activations (zero input rows, zero bias)
    (777, 64, 64, True, "negzero"),    # -0.0 input rows and bias
]


def _linear_data(M, K, N, leaky, special, gen):
    x = torch.randn(M, K, generator=gen)
    bound = 1.0 / math.sqrt(K)
    w = (torch.rand(N, K, generator=gen) * 2 - 1) * bound
    b = (torch.rand(N, generator=gen) * 2 - 1) * bound
    dy = torch.randn(M, N, generator=gen)
    if special == "zero":
        x[::7] = 0.0
        b.zero_()
    elif special == "negzero":
        x[::7] = -0.0
        x[3::7, ::2] = -0.0
        b.fill_(-0.0)
    if leaky:
        p = x.double() @ w.double().t() + b.double()
        near = (p.abs() < 1e-5 * float(p.abs().max())) & (p != 0)
        dy[near] = 0.0
    return x, w, b, dy


def _linear_legs(x, w, b, dy, leaky, want_dx=True):
    x = x.clone().requires_grad_(want_dx)
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.linear(x, w, b)
    if leaky:
        y = F.leaky_relu(y)
    (y * dy).sum().backward()
    return y.detach(), x.grad, w.grad, b.grad


@pytest.mark.parametrize("M,K,N,leaky,special", LINEAR_CASES)
def test_linear_against_float64(M, K, N, leaky, special):
    from speechseparation_amd import train
    gen = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x, w, b, dy = _linear_data(M, K, N, leaky, special, gen)
    r32 = _linear_legs(x, w, b, dy, leaky)
    r64 = _linear_legs(x.to(F64), w.to(F64), b.to(F64), dy.to(F64), leaky)
    xg = x.cuda().requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    y = train.LinearFunction.apply(xg, wg, bg, leaky)
    (y * dy.cuda()).sum().backward()
    torch.cuda.synchronize()
    label = "linear M=%d K=%d N=%d%s%s" % (M, K, N, " leaky" if leaky else "", " " + special if special else "")
    lay = _fmt([train.reduction_layout(M, N, K)])
    for name, g, a, c in zip(("y", "dx", "dw", "db"), (y, xg.grad, wg.grad, bg.grad), r32, r64):
        _check(label, lay, name, g, a, c, rows=name == "dw")
    if special:
        # the exactly-zero pre-activations took torch's slope (0.01) in the library too: dx of those rows = 0.01 dy W
        rows = slice(0, None, 7)
        want = 0.01 * dy[rows].double() @ w.double() if leaky else dy[rows].double() @ w.double()
        assert _err(xg.grad[rows], want) <= 3 * _err(r32[1][rows], want) + FLOOR


# a group of 25 jobs: three GEMM_GROUP launches, mixed widths, job 4 wants no input gradient
GROUP_DIMS = [(2, 2), (6, 64), (96, 96), (64, 128), (17, 65), (1, 1), (128, 64), (514, 514), (36, 36)] * 3
GROUP_DIMS = GROUP_DIMS[:25]
GROUP_NO_DX = 4


@pytest.mark.parametrize("leaky", [True, False])
def test_grouped_linear_against_float64(leaky):
    from speechseparation_amd import train
    assert len(GROUP_DIMS) > 2 * GEMM_GROUP
    M = 2000
    gen = torch.Generator().manual_seed(77 + leaky)
    data = [_linear_data(M, k, n, leaky, None, gen) for k, n in GROUP_DIMS]
    r32 = [_linear_legs(*d, leaky, want_dx=i != GROUP_NO_DX) for i, d in enumerate(data)]
    r64 = [_linear_legs(*(t.to(F64) for t in d), leaky, want_dx=i != GROUP_NO_DX) for i, d in enumerate(data)]
    xs = [d[0].cuda().requires_grad_(i != GROUP_NO_DX) for i, d in enumerate(data)]
    ws = [d[1].cuda().requires_grad_(True) for d in data]
    bs = [d[2].cuda().requires_grad_(True) for d in data]
    ys = train.GroupedLinearFunction.apply(leaky, len(data), *xs, *ws, *bs)
    sum((y * d[3].cuda()).sum() for y, d in zip(ys, data)).backward()
    torch.cuda.synchronize()
    assert xs[GROUP_NO_DX].grad is None
    for i, (k, n) in enumerate(GROUP_DIMS):
        label = "group job %d K=%d N=%d%s" % (i, k, n, " leaky" if leaky else "")
        lay = _fmt([train.reduction_layout(M, n, k)])
        got = (ys[i], xs[i].grad, ws[i].grad, bs[i].grad)
        for name, g, a, c in zip(("y", "dx", "dw", "db"), got, r32[i], r64[i]):
            if name == "dx" and i == GROUP_NO_DX:
                continue
            _check(label, lay, name, g, a, c, rows=name == "dw")


# ------------------------------------------------------------------------------------------ 3. AdamW
LR, BETAS, EPS, WD = 1e-3, (0.9, 0.999), 1e-8, 1e-2


def _adamw_f64(p, g, m, v, step):
    """torch.optim.AdamW (single tensor, not capturable) in its own operation order, in float64."""
    b1, b2 = BETAS
    p.mul_(1 - LR * WD)
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    denom = (v.sqrt() / math.sqrt(bc2)).add_(EPS)
    p.addcdiv_(m, denom, value=-(LR / bc1))


def _adam_sizes(kind):
    if kind == "sizes":
        return [1, 255, 1023, 1024, 1025, 70001, 0, 300]
    return [(37 * i) % 1100 + 1 for i in range(81 if kind == "81" else 161)]


@pytest.mark.parametrize("kind", ["sizes", "81", "161"])
def test_adamw_against_float64(kind):
    from speechseparation_amd import train
    sizes = _adam_sizes(kind)
    gen = torch.Generator().manual_seed(len(sizes))
    p0 = [torch.randn(n, generator=gen) for n in sizes]
    zero_grad = len(sizes) - 1                          # the last tensor's gradients are exactly 0 (v = 0: the denominator is eps)
    grads = [[torch.zeros(n) if i == zero_grad else torch.randn(n, generator=gen) * (0.1 + i % 3) for i, n in enumerate(sizes)]
             for _ in range(50)]

    p32 = [torch.nn.Parameter(t.clone()) for t in p0]
    opt32 = torch.optim.AdamW(p32, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, foreach=False)
    p64 = [t.to(F64) for t in p0]
    m64 = [torch.zeros_like(t) for t in p64]
    v64 = [torch.zeros_like(t) for t in p64]
    legs = {}
    for cap in (False, True):
        ps = [torch.nn.Parameter(t.cuda()) for t in p0]
        legs[cap] = (ps, train.AdamW(ps, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, capturable=cap))
    nonempty = [i for i, n in enumerate(sizes) if n > 0]
    assert len(legs[False][1].params) == len(nonempty)
    for step in range(1, 51):
        for i, g in enumerate(grads[step - 1]):
            p32[i].grad = g.clone()
            _adamw_f64(p64[i], g.to(F64), m64[i], v64[i], step)
            for ps, _ in legs.values():
                ps[i].grad = g.cuda()
        opt32.step()
        for _, opt in legs.values():
            opt.step()
        if step not in (1, 2, 50):
            continue
        torch.cuda.synchronize()
        (ph, oh), (pc, oc) = legs[False], legs[True]
        for j, i in enumerate(nonempty):
            # the host-argument path and the device-state path run the same kernel on the same bias corrections
            assert torch.equal(ph[i], pc[i]) and torch.equal(oh.m[j], oc.m[j]) and torch.equal(oh.v[j], oc.v[j]), (kind, step, i)
        for j, i in enumerate(nonempty):
            st = opt32.state[p32[i]]
            label = "adamw %s step %d tensor %d n=%d" % (kind, step, i, sizes[i])
            for name, g, a, c in (("p", ph[i], p32[i], p64[i]), ("m", oh.m[j], st["exp_avg"], m64[i]), ("v", oh.v[j], st["exp_avg_sq"], v64[i])):
                e_gpu, e_f32 = _err(g, c), _err(a, c)
                if i == zero_grad or i < 6 or i % 40 == 0:
                    print("%-34s %-22s %-6s e_gpu %.2e  e_f32 %.2e  bound %.2e" % (label, "", name, e_gpu, e_f32, 3 * e_f32 + FLOOR))
                assert e_gpu <= 3 * e_f32 + FLOOR, (label, name, e_gpu, e_f32)
        assert float(oh.v[nonempty.index(zero_grad)].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 4. the whole model
def _leaky_clearance(monkeypatch, fn):
    """Run fn with F.leaky_relu recording min |p| / max |p| of every call (how close a pre-activation comes to the kink)."""
    seen = []
    orig = F.leaky_relu

    def rec(t, *a, **k):
        d = t.detach().abs()
        seen.append(float(d.min() / d.max()) if d.numel() and float(d.max()) > 0 else 1.0)
        return orig(t, *a, **k)
    monkeypatch.setattr(F, "leaky_relu", rec)
    try:
        out = fn()
    finally:
        monkeypatch.setattr(F, "leaky_relu", orig)
    return out, min(seen)


def _cpu_loss(ref, mix, speech, dtype):
    win = torch.hann_window(2048, dtype=dtype)
    X = torch.stft(mix, n_fft=2048, hop_length=1024, return_complex=True, window=win)
    y = ref.forward_differentiable(torch.stack((X.real, X.imag), dim=2).reshape(mix.shape[0], 2050, -1))
    yc = y.reshape(y.shape[0], -1, 2, y.shape[2])
    Y = torch.complex(yc[:, :, 0, :], yc[:, :, 1, :])
    xt = torch.istft(Y, n_fft=2048, hop_length=1024, window=win)
    S = torch.stft(speech, n_fft=2048, hop_length=1024, return_complex=True, window=win)
    diffs = (xt - speech[:, :xt.shape[1]], Y.real - S.real, Y.imag - S.imag)
    loss = sum(d.abs().mean() for d in diffs)
    # (the imaginary parts of bins 0 and 1024 are 0 up to rounding in every leg; their gradient does not reach the model)
    kink = min(float(a.min() / a.max()) for a in (d.detach().abs() for d in (diffs[0], diffs[1], diffs[2][:, 1:-1])))
    return loss, kink


def test_whole_model_gradients_at_the_default_clip_against_float64(monkeypatch):
    """train.forward_train + the L1 tri-loss of train.train_loss on train.py's default clip (2 rows x 64 000 samples, T = 63):
    every parameter gradient against the CPU restatement in float64, per tensor."""
    from oracle.bsrnn_torch_cpu import TorchCpuBSRNN
    from speechseparation_amd import spec, train, weights
    from speechseparation_amd.bsrnn import BSRNN
    v = spec.generate_bandsplits()[0]
    n = 64000
    # how close the float64 pre-activations (LeakyReLU) and L1 terms come to their kinks, where a leg could take the other branch
    # of a derivative by rounding, is printed; the kernels are deterministic, so the fixed data passes or fails for good
    seed = 0
    sd = weights.synth_state_dict(None, seed=seed, lstm_gain=3.0)
    mix = torch.from_numpy(weights.synth_waveform(2, n, seed=100 + seed))
    speech = torch.from_numpy(weights.synth_waveform(2, n, seed=200 + seed))
    ref64 = TorchCpuBSRNN(sd, v, dtype=F64)
    with torch.no_grad():
        (_, kink), clear = _leaky_clearance(monkeypatch, lambda: _cpu_loss(ref64, mix.to(F64), speech.to(F64), F64))
    p64 = ref64.trainable()
    loss64, _ = _cpu_loss(ref64, mix.to(F64), speech.to(F64), F64)
    loss64.backward()
    ref32 = TorchCpuBSRNN(sd, v)
    p32 = ref32.trainable()
    loss32, _ = _cpu_loss(ref32, mix, speech, torch.float32)
    loss32.backward()

    m = BSRNN().train()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd.items()})
    m = m.to("cuda:0")
    loss, _ = train.train_loss(m, mix.cuda(), speech.cuda())
    loss.backward()
    torch.cuda.synchronize()
    label = "model seed %d T=63" % seed
    print("%s: pre-activation clearance %.1e, loss-term clearance %.1e" % (label, clear, kink))
    _check(label, "", "loss", loss.detach().reshape(1), loss32.detach().reshape(1), loss64.detach().reshape(1))
    count, worst = 0, (0.0, "")
    for name, p in m.named_parameters():
        if p.numel() == 0:
            continue
        g64, g32 = p64[name].grad, p32[name].grad
        assert p.grad is not None and g64 is not None, name
        e_gpu, e_f32 = _err(p.grad, g64), _err(g32, g64)
        worst = max(worst, (e_gpu / (3 * e_f32 + FLOOR), name))
        assert e_gpu <= 3 * e_f32 + FLOOR, (name, e_gpu, e_f32)
        count += 1
    print("%s: %d parameter gradients, largest e_gpu / bound %.2f (%s)" % (label, count, worst[0], worst[1]))
    assert count >= 280


# ------------------------------------------------------------------------------------------ 5. reproducibility at scale
def test_backward_at_the_bench_shape_is_bit_reproducible_across_scratch_growth():
    from speechseparation_amd import train
    torch.manual_seed(5)

    def layer(N, IN):
        x = torch.randn(N, 12, IN, device="cuda")
        w_ih, w_hh = torch.randn(2, 256, IN, device="cuda") * 0.2, torch.randn(2, 256, 64, device="cuda") * 0.2
        b = torch.randn(2, 256, device="cuda") * 0.1
        h, g, c = train.lstm_layer_forward(x, w_ih, w_hh, b)
        return x, h, g, c, torch.randn_like(h), w_ih, w_hh

    bench = layer(8064, 64)
    first = train.lstm_layer_backward(*bench)
    second = train.lstm_layer_backward(*bench)
    big = layer(12096, 128)                                  # more than 1.25 x the workspace: the training scratch grows
    train.lstm_layer_backward(*big)
    third = train.lstm_layer_backward(*bench)
    torch.cuda.synchronize()
    for name, a, b, c in zip(("dx", "dw_ih", "dw_hh", "db"), first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c), name


# ------------------------------------------------------------------------------------------ the layouts the cases reach
def test_shapes_reach_every_reduction_layout():
    """From the library's own query: the regimes of the chunk count, a single chunk, every count mod 4 and half-slab chunks."""
    from speechseparation_amd import train
    seen = []                                                # (M, tiles, chunks, rows per chunk)
    for N, L, IN, ndir, _ in LSTM_CASES:
        for n2 in (IN, 64):
            seen.append((N * L, 4 * (n2 // 64)) + train.reduction_layout(N * L, 256, n2))
    for M, K, N, *_ in LINEAR_CASES:
        seen.append((M, -(-N // 64) * -(-K // 64)) + train.reduction_layout(M, N, K))
    for K, N in GROUP_DIMS:
        seen.append((2000, -(-N // 64) * -(-K // 64)) + train.reduction_layout(2000, N, K))
    for M, tiles, chunks, rpc in seen:
        assert (chunks - 1) * rpc < M <= chunks * rpc and rpc % 16 == 0       # the chunks tile the rows
    regimes = {
        "M/512": lambda M, t: -(-M // 512),
        "cap": lambda M, t: LSTM_TRAIN_CHUNKS,
        "fill": lambda M, t: -(-1024 // t),
        "M/64": lambda M, t: -(-M // 64),
        "clamp": lambda M, t: LSTM_TRAIN_MAX_CHUNKS,
    }
    for name, value in regimes.items():
        # a case whose chunk count is this regime's value and none of the others'
        hits = [(M, t, c) for M, t, c, _ in seen
                if c == value(M, t) and all(c != other(M, t) for o, other in regimes.items() if o != name)]
        print("regime %-6s reached by (M, tiles, chunks) %s" % (name, hits[:3]))
        assert hits, name
    assert any(c == 1 for _, _, c, _ in seen)
    assert {c % 4 for _, _, c, _ in seen} == {0, 1, 2, 3}
    assert any(rpc % 32 == 16 and c > 1 for _, _, c, rpc in seen[:2 * len(LSTM_CASES)])      # half slabs in an LSTM case
    assert any(rpc % 32 == 16 and c > 1 for _, _, c, rpc in seen[2 * len(LSTM_CASES):])      # ... and in a Linear case
    assert train.reduction_layout(96768, 256, 64) == (252, 384)                                # the bench's band-axis dw_hh
    assert train.reduction_layout(96768, 256, 128) == (126, 768)                               # its layer-1 dw_ih
    assert train.reduction_layout(8064, 768, 768) == (16, 512)                                 # its 768 x 768 Linear layers
