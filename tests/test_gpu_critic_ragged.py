"""GPU: the committed critic on a padded batch (CommittedCritic.score_ragged / score_grad_ragged / score_fixed_ragged;
bsrnn_critic_score_ragged / _score_grad_ragged / _layer1_dx_ragged; csrc/critic_ragged_host.h): one clip owning the rectangle gives the
per-clip calls' bits, the padding is never read, integers are exact per clip, normal variates stay within the bounds
tests/test_critic_score_reference.py and tests/test_critic_grad_reference.py derive (per clip, against float64 on the clip ALONE, with a
clip whose dp1 is tiny beside its neighbour's), the chain against float64 autograd per clip, reproducibility, the range guard, the
refusals, and train_loss_ragged_critic: train_loss_ragged with the critic term.

The base batch: frames (793, 601, 603), rows (2, 1, 3), Tmax 793 - three frame tiles per row in the first layer's forward, two of them
dead for the four short rows, three position tiles in its dx, one of them dead for those rows."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import critic_reference as cr
import test_critic_grad_reference as gr
from test_gpu_critic import _within_stock, conv_backward, conv_forward
from test_gpu_critic_score import interleave

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EARG, ESTATE, ERANGE = 1, 2, 6                                                 # BSRNN_* of include/bsrnn_hip.h
FRAMES, ROWS, TMAX, R = (793, 601, 603), (2, 1, 3), 793, 6
_modules = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_critics():
    yield
    for _, cc in _modules.values():
        cc.close()
    _modules.clear()
    torch.cuda.empty_cache()


def _lib():
    from speechseparation_amd import _native, train
    return _native, _native.lib, train._context(torch.device(DEV))


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def critic(I, seed=5):
    from speechseparation_amd.discriminator import Discriminator
    if I not in _modules:
        D = Discriminator(I)
        D.load_state_dict(cr.synth_critic_state(I, seed=seed), strict=True)
        D = D.to(DEV)
        _modules[I] = (D, D.commit(grad=True))
    return _modules[I]


def set_first_layer(I, w, b=None):
    D, cc = critic(I)
    with torch.no_grad():
        D.layers[0].weight.copy_(w)
        if b is not None:
            D.layers[0].bias.copy_(b)
    cc.recommit(D)
    return D, cc


def ints(gen, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()


def clips_of(frames=FRAMES, rows=ROWS):
    """[(first row, rows, frames)] per clip."""
    out, r = [], 0
    for t, n in zip(frames, rows):
        out.append((r, n, t))
        r += n
    return out


def row_frames(frames=FRAMES, rows=ROWS):
    return [t for t, n in zip(frames, rows) for _ in range(n)]


def behind(x, lens, value):
    """A copy of x [R, ., L] with `value` at and behind lens[r] in row r."""
    x = x.clone()
    for r, t in enumerate(lens):
        x[r, :, t:] = value
    return x


def in_order(x, inter):
    return interleave(x) if inter else x


def back_order(dx, inter):
    from speechseparation_amd.discriminator import reference_channel_order
    return reference_channel_order(dx) if inter else dx


def _i32(v):
    return (ctypes.c_int32 * len(v))(*v)


# ------------------------------------------------------------------------------------------------ 1. the anchor
@pytest.mark.parametrize("inter", [False, True], ids=["planar", "interleaved"])
def test_one_clip_owning_the_rectangle_gives_the_per_clip_calls_bits(inter):
    """C = R, T = Tmax: the same plan, hence the same sums - any reordering shows."""
    D, cc = critic(66)
    cc.recommit(D)
    x = in_order(torch.randn((3, 66, TMAX), generator=_gen(1), device=DEV), inter)
    s, y1 = cc.score(x, interleaved=inter, return_y1=True)
    sr, y1r = cc.score_ragged(x, (TMAX,), (3,), interleaved=inter, return_y1=True)
    assert tuple(sr.shape) == (1,) and torch.equal(sr, s) and torch.equal(y1r, y1)
    half = torch.tensor([0.5], device=DEV)
    for gs in (None, half):
        s2, dx = cc.score_grad(x, interleaved=inter, gscale=gs)
        s2r, dxr = cc.score_grad_ragged(x, (TMAX,), (3,), interleaved=inter, gscale=gs)
        assert torch.equal(s2r, s) and torch.equal(s2, s) and torch.equal(dxr, dx)
    assert float(dx.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. the padding is never read
@pytest.mark.parametrize("inter", [False, True], ids=["planar", "interleaved"])
def test_padding_is_never_read(inter):
    D, cc = critic(66)
    cc.recommit(D)
    lens = row_frames()
    base = behind(torch.randn((R, 66, TMAX), generator=_gen(2), device=DEV), lens, 0.0)      # (the fill is the same in both orders)
    x0 = in_order(base, inter)
    s0, dx0 = cc.score_grad_ragged(x0, FRAMES, ROWS, interleaved=inter)
    sc0, y10 = cc.score_ragged(x0, FRAMES, ROWS, interleaved=inter, return_y1=True)
    assert torch.equal(sc0, s0) and bool(torch.isfinite(dx0).all()) and bool(torch.isfinite(s0).all())
    for r, t in enumerate(lens):
        assert bool((dx0[r, :, t:] == 0).all()) and float(dx0[r, :, :t].abs().max()) > 0     # zeros behind the frames, exactly
    for fill in (float("nan"), 1e30):
        xf = in_order(behind(base, lens, fill), inter)
        s, dx = cc.score_grad_ragged(xf, FRAMES, ROWS, interleaved=inter)
        sc, y1 = cc.score_ragged(xf, FRAMES, ROWS, interleaved=inter, return_y1=True)
        # the same bits: nothing behind the frames reached a product, and the guard was not raised (its re-run is the other path)
        assert torch.equal(s, s0) and torch.equal(dx, dx0) and torch.equal(sc, s0), fill
        for r, t in enumerate(lens):
            assert torch.equal(y1[r, :, :cr.t_out(t)], y10[r, :, :cr.t_out(t)])
    # another clip's content, and another clip's length (Tmax kept by clip 0), leave a clip alone
    other = base.clone()
    other[2:] = behind(torch.randn((4, 66, TMAX), generator=_gen(3), device=DEV), [700, 603, 603, 603], 0.0)
    s1, dx1 = cc.score_grad_ragged(in_order(other, inter), (793, 700, 603), ROWS, interleaved=inter)
    assert torch.equal(s1[0], s0[0]) and torch.equal(dx1[:2], dx0[:2]) and not torch.equal(s1[1:], s0[1:])
    other = base.clone()
    other[:2] = torch.randn((2, 66, TMAX), generator=_gen(4), device=DEV)
    s2, dx2 = cc.score_grad_ragged(in_order(other, inter), FRAMES, ROWS, interleaved=inter)
    assert torch.equal(s2[1:], s0[1:]) and torch.equal(dx2[2:], dx0[2:]) and not torch.equal(s2[0], s0[0])


# ------------------------------------------------------------------------------------------------ 3. integers
@pytest.mark.parametrize("I", [2, 7, 10, 66])
def test_integers_are_exact_per_clip(I):
    """Integers in [-2, 2] are fp16 values and every partial sum an integer below 2^24: per clip, y1 and the first layer's dx from an
    integer dp equal float64 evaluated on that clip ALONE, in both orders, over live and dead tiles; NaN stands behind every row's frames."""
    from speechseparation_amd.discriminator import layer1_dx_ragged
    g = _gen(40 + I)
    w, b = ints(g, (1024, I, 16)), ints(g, (1024,))
    _, cc = set_first_layer(I, w, b)
    lens = row_frames()
    x = behind(ints(g, (R, I, TMAX)), lens, float("nan"))
    dp = behind(ints(g, (R, 1024, cr.t_out(TMAX))), [cr.t_out(t) for t in lens], 0.0)
    for inter in (False, True) if I % 2 == 0 else (False,):
        _, y1 = cc.score_ragged(in_order(x, inter), FRAMES, ROWS, interleaved=inter, return_y1=True)
        dx = back_order(layer1_dx_ragged(cc, dp, TMAX, FRAMES, ROWS, interleaved=inter), inter)
        assert tuple(y1.shape) == (R, 1024, cr.t_out(TMAX)) and tuple(dx.shape) == (R, I, TMAX)
        for r0, n, t in clips_of():
            xc = x[r0:r0 + n, :, :t].cpu().double()
            ref = cr.leaky32(F.conv1d(xc, w.cpu().double(), b.cpu().double(), stride=3))
            assert torch.equal(y1[r0:r0 + n, :, :cr.t_out(t)].cpu().double(), ref), (I, inter, r0)
            g64 = F.conv_transpose1d(dp[r0:r0 + n, :, :cr.t_out(t)].cpu().double(), w.cpu().double(), stride=3)
            want = F.pad(g64, (0, TMAX - g64.shape[2]))                           # zeros behind the last window and behind the frames
            assert torch.equal(dx[r0:r0 + n].cpu().double(), want), (I, inter, r0)


# ------------------------------------------------------------------------------------------------ 4. rounding
@pytest.mark.parametrize("I", [10, 66])
def test_rounding_within_the_proven_bounds_per_clip(I):
    """Normal variates.  y1: every element within (16 I + 14) u S of float64 on the clip alone (tests/test_critic_score_reference.py;
    the bound holds for any order of the sum, so for the rectangle's slab count too).  dx: every element within
    tests/test_critic_grad_reference.py's dx_bound of float64 ON THE CLIP ALONE - its m is the clip's own max |dp1|.  Clip 1's dp1 is
    2^-20 times its neighbours' and clip 2's 2^-44 times: tests/test_critic_ragged_reference.py shows that one exponent per batch still
    meets the bound at 2^-20 and misses it at 2^-44."""
    from speechseparation_amd.discriminator import layer1_dx_ragged
    rng = np.random.default_rng(50 + I)
    lens = row_frames()
    x = rng.standard_normal((R, I, TMAX)).astype(np.float32)
    w, b = rng.standard_normal((1024, I, 16)).astype(np.float32), rng.standard_normal((1024,)).astype(np.float32)
    _, cc = set_first_layer(I, torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV))
    xd = behind(torch.from_numpy(x).to(DEV), lens, float("nan"))
    wg = gr.weights(rng, I)
    dp = (1e-8 * rng.standard_normal((R, 1024, cr.t_out(TMAX)))).astype(np.float32)
    dp[2] *= np.float32(2.0 ** -20)
    dp[3:] *= np.float32(2.0 ** -44)
    for r, t in enumerate(lens):
        dp[r, :, cr.t_out(t):] = 0
    for inter in (False, True):
        _, y1 = cc.score_ragged(in_order(xd, inter), FRAMES, ROWS, interleaved=inter, return_y1=True)
        for r0, n, t in clips_of():
            xc = torch.from_numpy(x[r0:r0 + n, :, :t])
            ref = cr.layer(xc, torch.from_numpy(w), torch.from_numpy(b), torch.zeros(n, 1024, cr.t_out(t)), leaky=True, want_dx=False)
            lim = (16 * I + 14) * cr.U * ref["S_y"]
            err = (y1[r0:r0 + n, :, :cr.t_out(t)].cpu().double() - ref["y"]).abs()
            print("y1, I = %d, clip at row %d, %s: worst error / bound = %.3f" % (I, r0, "interleaved" if inter else "planar", float((err / lim).max())))
            assert bool((err <= lim).all())
    _, cc = set_first_layer(I, torch.from_numpy(wg).to(DEV))
    for inter in (False, True):
        dx = back_order(layer1_dx_ragged(cc, torch.from_numpy(dp).to(DEV), TMAX, FRAMES, ROWS, interleaved=inter), inter).cpu().double().numpy()
        for r0, n, t in clips_of():
            d = dp[r0:r0 + n, :, :cr.t_out(t)]
            ref, lim = gr.dx_float64(wg, d, t), gr.dx_bound(wg, d, t)
            err = np.abs(dx[r0:r0 + n, :, :t] - ref)
            print("dx, I = %d, clip at row %d, %s: worst error / bound = %.4f" % (
                I, r0, "interleaved" if inter else "planar", float((err / np.maximum(lim, np.finfo(np.float64).tiny)).max())))
            assert bool((err <= lim).all())
            assert float(np.abs(dx[r0:r0 + n, :, :t]).max()) > 0 and bool((dx[r0:r0 + n, :, t:] == 0).all())      # not flushed; zeros behind


# ------------------------------------------------------------------------------------------------ 5. the chain
def _chain_reference(sd, I, x):
    ref64, ref32 = cr.CriticF64(I), cr.CriticF64(I, dtype=torch.float32)
    ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ref32.load_state_dict(sd, strict=True)
    for p in list(ref64.parameters()) + list(ref32.parameters()):
        p.requires_grad_(False)
    x64, x32 = x.double().requires_grad_(True), x.clone().requires_grad_(True)
    s64, s32 = ref64(x64), ref32(x32)
    s64.sum().backward()
    s32.sum().backward()
    return s64.detach(), s32.detach(), x64.grad, x32.grad


def test_score_and_dx_per_clip_against_float64_autograd():
    """66 channels, per clip against float64 autograd of the clip alone by the module's rule (stock fp32 autograd's error x 4 + 2^-23);
    gscale per clip; score_fixed_ragged's backward."""
    sd = cr.synth_critic_state(66, seed=5)
    D, cc = critic(66)
    D.load_state_dict(sd, strict=True)
    cc.recommit(D)
    lens = row_frames()
    x = torch.from_numpy(np.random.default_rng(8).standard_normal((R, 66, TMAX)).astype(np.float32))
    xd = behind(x.to(DEV), lens, float("nan"))
    s, dx = cc.score_grad_ragged(xd, FRAMES, ROWS)
    assert tuple(s.shape) == (3,) and tuple(dx.shape) == (R, 66, TMAX) and not s.requires_grad and not dx.requires_grad
    assert torch.equal(s, cc.score_ragged(xd, FRAMES, ROWS))
    for c, (r0, n, t) in enumerate(clips_of()):
        s64, s32, g64, g32 = _chain_reference(sd, 66, x[r0:r0 + n, :, :t])
        _within_stock("score of clip %d" % c, s[c:c + 1].cpu(), s64, s32)
        _within_stock("dx of clip %d" % c, dx[r0:r0 + n, :, :t].cpu(), g64, g32)
        assert bool((dx[r0:r0 + n, :, t:] == 0).all())
    gs = torch.tensor([0.5, 1.0, 0.0], device=DEV)
    s_g, dx_g = cc.score_grad_ragged(xd, FRAMES, ROWS, gscale=gs)
    assert torch.equal(s_g, s)
    assert torch.equal(dx_g[:2], dx[:2] * 0.5) and torch.equal(dx_g[2:3], dx[2:3]) and bool((dx_g[3:] == 0).all())
    xa = behind(x.to(DEV), lens, 0.0).requires_grad_(True)
    sf = cc.score_fixed_ragged(xa, FRAMES, ROWS)
    assert torch.equal(sf.detach(), s) and sf.requires_grad
    sf.sum().backward()
    assert torch.equal(xa.grad, dx)                                           # the same dx bit for bit
    si, dxi = cc.score_grad_ragged(interleave(xd), FRAMES, ROWS, interleaved=True)
    assert torch.equal(si, s) and torch.equal(back_order(dxi, True), dx)
    with pytest.raises(ValueError, match="clip 1 has 600 frames"):
        cc.score_grad_ragged(xd, (793, 600, 603), ROWS)
    with pytest.raises(ValueError, match="gscale"):
        cc.score_grad_ragged(xd, FRAMES, ROWS, gscale=torch.ones(2, device=DEV))
    plain = D.commit()
    try:
        assert torch.equal(plain.score_ragged(xd, FRAMES, ROWS), s)
        with pytest.raises(ValueError, match="grad=True"):
            plain.score_grad_ragged(xd, FRAMES, ROWS)
    finally:
        plain.close()


# ------------------------------------------------------------------------------------------------ 6. determinism, the guard, refusals
def _exact_chain_ragged(D, x, scores, gscale=None):
    """dx of the exact chain through the library's exposed layer calls on the zero-padded planar rectangle (the kernels the re-run
    launches, at the rectangle's shape), from the call's own scores: per clip the tail's gradient in the kernel's order of operations,
    zeros behind a row's T4_r, then bsrnn_critic_conv_backward layer by layer."""
    convs = [m for m in D.layers if isinstance(m, torch.nn.Conv1d)]
    ws, bs = [c.weight.detach() for c in convs], [c.bias.detach() for c in convs]
    ys, h = [], x
    for l in range(4):
        h = conv_forward(h, ws[l], bs[l], l < 3)
        ys.append(h)
    T4max = ys[3].shape[2]
    lw = D.layers2[0].weight.detach().reshape(-1)
    dev = lambda v: torch.tensor(float(v), device=DEV)                         # noqa: E731  (tensor / tensor: a true division)
    dy = torch.zeros((R, 32, T4max), device=DEV)
    for c, (r0, n, t) in enumerate(clips_of()):
        T4 = cr.t_out(cr.t_out(cr.t_out(cr.t_out(t))))
        s = scores[c]
        gp = (((dev(1.0 if gscale is None else gscale[c]) * ((1.0 - s) * s)) * lw) / dev(n)) / dev(T4)
        dy[r0:r0 + n, :, :T4] = gp.reshape(1, -1, 1)
    for l in (3, 2, 1, 0):
        dy, _, _ = conv_backward(x if l == 0 else ys[l - 1], ws[l], ys[l], dy, l < 3)
    return dy


def test_reproducible_allocation_free_and_the_range_guard():
    native, lib, ctx = _lib()
    sd = cr.synth_critic_state(66, seed=5)
    D, cc = critic(66)
    D.load_state_dict(sd, strict=True)
    cc.recommit(D)
    lens = row_frames()
    xc = torch.from_numpy(np.random.default_rng(9).standard_normal((R, 66, TMAX)).astype(np.float32))
    x = behind(xc.to(DEV), lens, 0.0)
    s0, dx0 = cc.score_grad_ragged(x, FRAMES, ROWS)
    sc0 = cc.score_ragged(x, FRAMES, ROWS)
    torch.cuda.synchronize()
    before = lib.bsrnn_debug_counter(0)
    s1, dx1 = cc.score_grad_ragged(x, FRAMES, ROWS)
    sc1 = cc.score_ragged(x, FRAMES, ROWS)
    torch.cuda.synchronize()
    assert lib.bsrnn_debug_counter(0) == before                                # a second call of the shape allocates nothing
    assert torch.equal(s1, s0) and torch.equal(dx1, dx0) and torch.equal(sc1, sc0) and torch.equal(sc0, s0)
    assert not torch.equal(dx0, _exact_chain_ragged(D, x, s0))                 # (the fp16x2 path is the other path)
    # 1e5 behind a row's frames does nothing; inside a row the whole call runs again on the exact chain
    assert lib.bsrnn_get_range_policy(ctx) == native.RANGE_EXACT
    x_pad = behind(x, lens, 1e5)
    s2, dx2 = cc.score_grad_ragged(x_pad, FRAMES, ROWS)
    assert torch.equal(s2, s0) and torch.equal(dx2, dx0)
    x_hot = x.clone()
    x_hot[3, 3, 100] = 1e5
    s, dx = cc.score_grad_ragged(x_hot, FRAMES, ROWS)                          # rc 0, and the exact kernels' bits
    assert torch.equal(dx, _exact_chain_ragged(D, x_hot, s)) and torch.equal(s, cc.score_ragged(x_hot, FRAMES, ROWS))
    x_hot_pad = behind(x_hot, lens, float("nan"))                              # (the exact chain reads a planar x as it lies: NaN stays behind)
    s_n, dx_n = cc.score_grad_ragged(x_hot_pad, FRAMES, ROWS)
    assert torch.equal(s_n, s) and torch.equal(dx_n, dx)
    si, dxi = cc.score_grad_ragged(interleave(x_hot_pad), FRAMES, ROWS, interleaved=True)      # a zero-padded planar copy in, a scatter out
    assert torch.equal(si, s) and torch.equal(back_order(dxi, True), dx)
    for c, (r0, n, t) in enumerate(clips_of()):
        s64, s32, _, _ = _chain_reference(sd, 66, x_hot.cpu()[r0:r0 + n, :, :t])
        _within_stock("exact score of clip %d" % c, s[c:c + 1].cpu(), s64, s32)
    gs = torch.tensor([0.5, 1.0, 0.0], device=DEV)
    s_g, dx_g = cc.score_grad_ragged(x_hot, FRAMES, ROWS, gscale=gs)
    assert torch.equal(s_g, s) and torch.equal(dx_g, _exact_chain_ragged(D, x_hot, s, gs.tolist()))
    s3, dx3 = cc.score_grad_ragged(x, FRAMES, ROWS)                            # the guard is taken: the next call is fp16x2 again
    assert torch.equal(s3, s0) and torch.equal(dx3, dx0)
    native.check(lib.bsrnn_set_range_policy(ctx, native.RANGE_DEFERRED))
    try:
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        cc.score_grad_ragged(x_pad, FRAMES, ROWS)
        cc.score_ragged(x_pad, FRAMES, ROWS)
        assert lib.bsrnn_sync(ctx, stream) == 0                                # behind the frames: no guard
        cc.score_grad_ragged(x_hot, FRAMES, ROWS)                              # asynchronous, rc 0
        assert lib.bsrnn_sync(ctx, stream) == ERANGE and "65504" in lib.bsrnn_last_error().decode()
        assert lib.bsrnn_sync(ctx, None) == 0                                  # reported once
        cc.score_ragged(x_hot, FRAMES, ROWS)
        assert lib.bsrnn_sync(ctx, stream) == ERANGE
    finally:
        native.check(lib.bsrnn_set_range_policy(ctx, native.RANGE_EXACT))
    # a weight beyond the fp16 range: that object runs the exact chain directly
    w = D.layers[0].weight.detach().clone()
    w_hot = w.clone()
    w_hot[5, 1, 2] = 7e4
    D, cc = set_first_layer(66, w_hot)
    s4, dx4 = cc.score_grad_ragged(x, FRAMES, ROWS)
    assert torch.equal(dx4, _exact_chain_ragged(D, x, s4)) and bool(torch.isfinite(dx4).all())
    set_first_layer(66, w)


def test_argument_refusals():
    from speechseparation_amd import spec
    native, lib, ctx = _lib()
    nx, ny1 = R * 66 * TMAX, R * 1024 * cr.t_out(TMAX)
    S = R * 67 * TMAX                                                          # (the blocks lie apart for the 67-channel object too)
    buf = torch.zeros(2 * S + ny1 + 4096, device=DEV)
    before = buf.clone()
    at = lambda n: ctypes.c_void_p(buf.data_ptr() + 4 * n)                     # noqa: E731
    x, dx, y1, out, gs = at(0), at(S), at(2 * S), at(2 * S + ny1 + 4), at(2 * S + ny1 + 16)
    null = ctypes.c_void_p()
    D, cc = critic(66)
    cc.recommit(D)
    fr, rw = _i32(FRAMES), _i32(ROWS)

    def refused(rc, code, word):
        msg = lib.bsrnn_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    def all3(code, word, h=cc._h, x=x, R_=R, Tmax=TMAX, fr=fr, rw=rw, n=3, order=0, out=out, dx=dx, gs=gs, y1=y1):
        refused(lib.bsrnn_critic_score_ragged(h, x, R_, Tmax, fr, rw, n, order, out, y1, None), code, word)
        refused(lib.bsrnn_critic_score_grad_ragged(h, x, R_, Tmax, fr, rw, n, order, gs, out, dx, None), code, word)
        refused(lib.bsrnn_critic_layer1_dx_ragged(h, y1, R_, Tmax, fr, rw, n, order, dx, None), code, word)

    def sizes(h):
        all3(EARG, "n_clips", h=h, n=0)
        all3(EARG, "clip 1 has 0 rows", h=h, rw=_i32((2, 0, 4)))
        all3(EARG, "clip 2 has 600 frames", h=h, fr=_i32((793, 601, 600)))
        all3(EARG, "clip 0 has 794 frames", h=h, fr=_i32((794, 601, 603)))
        all3(EARG, "sum to R", h=h, R_=7)
        all3(EARG, "x_order", h=h, order=2)
        all3(EARG, "x_order", h=h, order=-1)
        all3(EARG, "2^31", h=h, R_=1 << 20, rw=_i32((1 << 20,)), fr=_i32((793,)), n=1)
        all3(EARG, "2^31", h=h, Tmax=1 << 30)
        refused(lib.bsrnn_critic_score_grad_ragged(h, x, R, TMAX, fr, rw, 3, 0, gs, out, at(nx - 1), None), EARG, "dx_dev overlaps x_dev")
        refused(lib.bsrnn_critic_score_grad_ragged(h, x, R, TMAX, fr, rw, 3, 0, gs, at(S + 7), dx, None), EARG, "dx_dev overlaps scores_dev")
        refused(lib.bsrnn_critic_score_grad_ragged(h, x, R, TMAX, fr, rw, 3, 0, gs, at(100), dx, None), EARG, "scores_dev overlaps x_dev")
        refused(lib.bsrnn_critic_score_grad_ragged(h, x, R, TMAX, fr, rw, 3, 0, at(S + 9), out, dx, None), EARG, "gscale_dev overlaps")
        refused(lib.bsrnn_critic_score_grad_ragged(h, x, R, TMAX, fr, rw, 3, 0, at(2 * S + ny1 + 6), out, dx, None), EARG, "gscale_dev overlaps")
        refused(lib.bsrnn_critic_score_ragged(h, x, R, TMAX, fr, rw, 3, 0, at(100), y1, None), EARG, "scores_dev overlaps x_dev")
        refused(lib.bsrnn_critic_score_ragged(h, x, R, TMAX, fr, rw, 3, 0, out, at(nx - 1), None), EARG, "y1_dev overlaps x_dev")
        refused(lib.bsrnn_critic_score_ragged(h, x, R, TMAX, fr, rw, 3, 0, at(2 * S + 5), y1, None), EARG, "scores_dev overlaps y1_dev")
        refused(lib.bsrnn_critic_layer1_dx_ragged(h, y1, R, TMAX, fr, rw, 3, 0, at(2 * S - 1), None), EARG, "dx_dev overlaps dp_dev")

    all3(EARG, "null", h=null)
    all3(EARG, "null", fr=None)
    all3(EARG, "null", rw=None)
    all3(EARG, "null", x=null, y1=null)
    refused(lib.bsrnn_critic_score_ragged(cc._h, x, R, TMAX, fr, rw, 3, 0, null, y1, None), EARG, "null")
    refused(lib.bsrnn_critic_score_grad_ragged(cc._h, x, R, TMAX, fr, rw, 3, 0, gs, null, dx, None), EARG, "null")
    refused(lib.bsrnn_critic_score_grad_ragged(cc._h, x, R, TMAX, fr, rw, 3, 0, gs, out, null, None), EARG, "null")
    refused(lib.bsrnn_critic_layer1_dx_ragged(cc._h, y1, R, TMAX, fr, rw, 3, 0, null, None), EARG, "null")
    sizes(cc._h)
    lay = (ctypes.c_int64 * 14)()
    refused(lib.bsrnn_critic_ragged_layout(66, R, TMAX, fr, rw, 3, None), EARG, "layout")
    refused(lib.bsrnn_critic_ragged_layout(66, R, TMAX, None, rw, 3, lay), EARG, "null")
    refused(lib.bsrnn_critic_ragged_layout(0, R, TMAX, fr, rw, 3, lay), EARG, "in_channels")
    assert lib.bsrnn_critic_ragged_layout(66, R, TMAX, fr, rw, 3, lay) == 0 and list(lay)[6:10] == [3, 14, 3, 14]
    # an odd channel count has no interleaved form; before the first commit; committed but without the gradient
    odd = ctypes.c_void_p()
    native.check(lib.bsrnn_critic_create(ctx, 67, ctypes.byref(odd)))
    try:
        all3(EARG, "odd", h=odd, order=1)
        all3(ESTATE, "commit", h=odd)
    finally:
        lib.bsrnn_critic_destroy(odd)
    plain = D.commit()
    try:
        refused(lib.bsrnn_critic_score_grad_ragged(plain._h, x, R, TMAX, fr, rw, 3, 0, gs, out, dx, None), ESTATE, "enable_grad")
        refused(lib.bsrnn_critic_layer1_dx_ragged(plain._h, y1, R, TMAX, fr, rw, 3, 0, dx, None), ESTATE, "enable_grad")
    finally:
        plain.close()
    # a host-only context: the arguments first, then BSRNN_ESTATE
    v = spec.generate_bandsplits()[0]
    host = ctypes.c_void_p()
    native.check(lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(host)))
    hk = ctypes.c_void_p()
    try:
        native.check(lib.bsrnn_critic_create(host, 66, ctypes.byref(hk)))
        sizes(hk)
        all3(ESTATE, "host-only", h=hk)
    finally:
        lib.bsrnn_critic_destroy(hk)
        lib.bsrnn_destroy(host)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                            # nothing was launched
    xs = torch.randn((R, 66, TMAX), generator=_gen(9), device=DEV)
    s, g = cc.score_grad_ragged(xs, FRAMES, ROWS)
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(g).all())     # the object is untouched by the refusals


# ------------------------------------------------------------------------------------------------ 7. training
def test_train_loss_ragged_with_a_committed_critic(sd_default):
    """The synthetic separator at 2050 channels, two mono clips of 601 and 640 frames.  losses[c] = the plain ragged loss + cc.score of
    that clip's spectrum alone within one fp32 rounding of the sum, the gradients those of discriminator=None bit for bit; with
    adversarial=True, per parameter tensor max |g_ragged - g_loop| <= 1e-3 max |g_loop - g_plain| (g_loop: the sum of the per-clip
    train_loss(adversarial=True) gradients with the same object) - the plumbing condition of
    test_adversarial_train_loss_with_a_committed_critic: a wrong factor or order gives O(1)."""
    from speechseparation_amd import train, weights
    from speechseparation_amd.bsrnn import BSRNN
    from speechseparation_amd.discriminator import Discriminator
    lens = [600 * 1024, 639 * 1024]
    m = BSRNN()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd_default.items()})
    m = m.to(DEV).train()
    mix = torch.from_numpy(weights.synth_waveform(2, lens[1], seed=31)).to(DEV)
    speech = torch.from_numpy(weights.synth_waveform(2, lens[1], seed=32)).to(DEV)
    D = Discriminator(2050)
    D.load_state_dict(cr.synth_critic_state(2050, seed=17), strict=True)
    D = D.to(DEV)
    cc = D.commit(grad=True)
    plain = D.commit()

    def grads(fn):
        for p in m.parameters():
            p.grad = None
        out = fn()
        return out, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    def ragged(**kw):
        losses, _, _ = (train.train_loss_ragged_critic if kw else train.train_loss_ragged)(m, mix, speech, lens, **kw)
        losses.sum().backward()
        return losses.detach()

    def loop():
        for c, n in enumerate(lens):
            loss, _ = train.train_loss(m, mix[c:c + 1, :n], speech[c:c + 1, :n], discriminator=cc, adversarial=True)
            loss.backward()

    try:
        l0, g0 = grads(ragged)
        l1, g1 = grads(lambda: ragged(discriminator=cc))
        assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)       # a constant: the same gradients bit for bit
        for c, n in enumerate(lens):
            with torch.no_grad():
                y = train.forward_train(m, train.stft(mix[c:c + 1, :n]))
                score = cc.score(y, interleaved=True).reshape(())
            want = l0[c] + score
            print("clip %d: loss %.9g, plain %.9g + score %.9g, difference %.3e" % (c, float(l1[c]), float(l0[c]), float(score), float(l1[c] - want)))
            assert float(score) != 0.0 and float((l1[c] - want).abs()) <= 2.0 ** -23 * float(want.abs())
        l2, g2 = grads(lambda: ragged(discriminator=cc, adversarial=True))
        assert torch.equal(l2, l1)
        _, g3 = grads(loop)
        assert set(g2) == set(g3) == set(g0) and any(not torch.equal(g0[k], g2[k]) for k in g0)
        worst = 0.0
        for k in g0:
            moved = float((g3[k] - g0[k]).abs().max())
            off = float((g2[k] - g3[k]).abs().max())
            if moved > 0:
                worst = max(worst, off / moved)
            assert off <= 1e-3 * moved, (k, off, moved)
        print("worst max|g_ragged - g_loop| / max|g_loop - g_plain| over the parameter tensors: %.3e" % worst)
        with pytest.raises(ValueError, match="adversarial"):
            train.train_loss_ragged_critic(m, mix, speech, lens, discriminator=plain, adversarial=True)
        with pytest.raises(ValueError, match="adversarial"):
            train.train_loss_ragged_critic(m, mix, speech, lens, adversarial=True)
        with pytest.raises(ValueError, match="CommittedCritic"):
            train.train_loss_ragged_critic(m, mix, speech, lens, discriminator=D)
        with pytest.raises(ValueError, match="clip 0 has 600 frames"):
            train.train_loss_ragged_critic(m, mix, speech, [599 * 1024 + 5, lens[1]], discriminator=cc)
    finally:
        cc.close()
        plain.close()
