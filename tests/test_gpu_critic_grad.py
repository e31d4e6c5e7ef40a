"""GPU: the committed critic's gradient (Discriminator.commit(grad=True); bsrnn_critic_enable_grad / _score_grad / _layer1_dx;
csrc/critic_grad.hip): the fp16x2 first-layer dx exactly on integer data and within the bound tests/test_critic_grad_reference.py derives
on normal variates and on a realistically tiny dp, the whole chain against float64 autograd by the module's rule, both input orders,
reproducibility and the snapshot, the range guard and its exact re-run, the adversarial training step and the argument refusals."""
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
_modules = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_critics():
    """The shared modules and their committed critics (two images and a snapshot each) go with this file."""
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
    """One Discriminator(I) on the device with synthetic weights and its CommittedCritic with the gradient, shared by the tests (a test
    that changes the weights recommits)."""
    from speechseparation_amd.discriminator import Discriminator
    if I not in _modules:
        D = Discriminator(I)
        if I <= 2050:
            D.load_state_dict(cr.synth_critic_state(I, seed=seed), strict=True)
        D = D.to(DEV)
        _modules[I] = (D, D.commit(grad=True))
    return _modules[I]


def set_first_layer(I, w):
    D, cc = critic(I)
    with torch.no_grad():
        D.layers[0].weight.copy_(w)
    cc.recommit(D)
    return D, cc


def ints(gen, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=DEV).float()


def dx_ref64(w, dp, T):
    """The definition in float64 on the CPU: conv_transpose1d, zeros behind the last window."""
    g = F.conv_transpose1d(dp.cpu().double(), w.cpu().double(), stride=3)
    return F.pad(g, (0, T - g.shape[2]))


def both_orders(cc, dp, T, even):
    """layer1_dx in planar order, and - where the channel count allows - in interleaved order, mapped back and compared bit for bit."""
    from speechseparation_amd.discriminator import layer1_dx, reference_channel_order
    dx = layer1_dx(cc, dp, T)
    if even:
        dxi = layer1_dx(cc, dp, T, interleaved=True)
        assert torch.equal(reference_channel_order(dxi), dx)
        assert torch.equal(interleave(dx), dxi)
    return dx


# ------------------------------------------------------------------------------------------------ 1. integers
@pytest.mark.parametrize("I", [2, 7, 10, 66])
def test_integers_are_exact(I):
    """Integers in [-2, 2] are fp16 values (dp scaled by 2^13 or 2^14 still is), so every second piece is zero and every partial sum an
    integer times the scale, at most 1024 * 6 products of magnitude 4: dx equals float64 - over a partial channel tile (2, 7, 10, 66 are
    no multiples of 8), one and two position tiles with the 5-frame halo between them (601 .. 603: two, 793: three), the trailing
    positions of 602 and 603 that no window reaches, and both row orders."""
    g = _gen(I)
    w = ints(g, (1024, I, 16))
    _, cc = set_first_layer(I, w)
    for T in (601, 602, 603, 793):
        for C in (1, 3):
            dp = ints(g, (C, 1024, cr.t_out(T)))
            dx = both_orders(cc, dp, T, I % 2 == 0)
            assert tuple(dx.shape) == (C, I, T)
            assert torch.equal(dx.cpu().double(), dx_ref64(w, dp, T)), (I, T, C)
            reach = 3 * (cr.t_out(T) - 1) + 16                                  # behind the last window: zeros
            assert T - reach == {601: 0, 602: 1, 603: 2, 793: 0}[T] and bool((dx[:, :, reach:] == 0).all())


def test_second_pieces_are_exact():
    """W = a + b 2^-12 (a, b in {-1, 0, 1}) needs the second piece; with dp in {-1, 0, 1} every sum is representable (checked), so
    dx equals float64 - a lost or misplaced second piece shows bit for bit (tests/test_critic_grad_reference.py)."""
    g = _gen(77)
    I, T = 10, 602
    w = ints(g, (1024, I, 16), -1, 1) + ints(g, (1024, I, 16), -1, 1) * 2.0 ** -12
    dp = ints(g, (2, 1024, cr.t_out(T)), -1, 1)
    ref = dx_ref64(w, dp, T)
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) < 2.0 ** 12
    _, cc = set_first_layer(I, w)
    assert torch.equal(both_orders(cc, dp, T, True).cpu().double(), ref)


def test_integers_at_full_width_equal_the_exact_kernel():
    """4098 channels, 601 frames, 2 rows - 513 x 2 x 2 workgroups, the last channel tile partial: dx equals
    bsrnn_critic_conv_backward's with the identity activation bit for bit (both exact), compared on the device."""
    from speechseparation_amd.discriminator import grad_layout
    g = _gen(4098)
    w, dp = ints(g, (1024, 4098, 16)), ints(g, (2, 1024, 196))
    _, cc = set_first_layer(4098, w)
    lay = grad_layout(4098, 2, 601)
    print("layout", lay)
    assert lay["i_tiles"] * lay["s_tiles"] * 2 == 2052 and 4098 % lay["tile_channels"] != 0
    want, _, _ = conv_backward(torch.zeros((2, 4098, 601), device=DEV), w, None, dp, False)
    assert torch.equal(both_orders(cc, dp, 601, True), want)


# ------------------------------------------------------------------------------------------------ 2. rounding
@pytest.mark.parametrize("case", ["normal-66-601", "normal-10-793", "small-dp-10-601"])
def test_rounding_within_the_proven_bound(case):
    """Every element of dx within the bound of tests/test_critic_grad_reference.py (dx_bound: (n + 14) u S and the subnormal terms) of
    float64, in both orders.  small-dp: dp ~ 1e-8 N(0, 1), the second row 2^-20 times smaller - without the scale this misses the bound
    by three orders of magnitude (shown there)."""
    kind, I, T = case.rsplit("-", 2)
    I, T = int(I), int(T)
    rng = np.random.default_rng(31 + I)
    w = gr.weights(rng, I) if kind == "small-dp" else rng.standard_normal((1024, I, 16)).astype(np.float32)
    dp = gr.small_dp(rng, 2, cr.t_out(T)) if kind == "small-dp" else rng.standard_normal((2, 1024, cr.t_out(T))).astype(np.float32)
    ref, lim = gr.dx_float64(w, dp, T), gr.dx_bound(w, dp, T)
    _, cc = set_first_layer(I, torch.from_numpy(w).to(DEV))
    dx = both_orders(cc, torch.from_numpy(dp).to(DEV), T, True).cpu().double().numpy()
    err = np.abs(dx - ref)
    print("%s: worst error / bound = %.4f" % (case, float((err / np.maximum(lim, np.finfo(np.float64).tiny)).max())))
    assert bool((err <= lim).all())
    assert float(np.abs(dx[1]).max()) > 0 if kind == "small-dp" else True      # (the small row is not flushed)


def test_zero_dp_gives_zero():
    from speechseparation_amd.discriminator import layer1_dx
    _, cc = critic(66)
    dx = layer1_dx(cc, torch.zeros((1, 1024, 196), device=DEV), 601)
    assert bool((dx == 0).all())


# ------------------------------------------------------------------------------------------------ 3. the chain
def _chain_reference(sd, I, x):
    ref64, ref32 = cr.CriticF64(I), cr.CriticF64(I, dtype=torch.float32)
    ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ref32.load_state_dict(sd, strict=True)
    for p in list(ref64.parameters()) + list(ref32.parameters()):
        p.requires_grad_(False)
    x64, x32 = x.double().requires_grad_(True), x.clone().requires_grad_(True)
    ref64(x64).sum().backward()
    ref32(x32).sum().backward()
    return x64.grad, x32.grad


@pytest.mark.parametrize("T", [601, 684])
def test_score_grad_against_float64_autograd(T):
    from speechseparation_amd.discriminator import Discriminator, reference_channel_order
    sd = cr.synth_critic_state(66, seed=5)
    D = Discriminator(66)
    D.load_state_dict(sd, strict=True)
    cc = D.to(DEV).commit(grad=True)
    assert cc.has_grad
    x = torch.from_numpy(np.random.default_rng(T).standard_normal((2, 66, T)).astype(np.float32))
    g64, g32 = _chain_reference(sd, 66, x)
    xd = x.to(DEV)
    s, dx = cc.score_grad(xd)
    assert tuple(s.shape) == (1,) and tuple(dx.shape) == (2, 66, T) and not s.requires_grad and not dx.requires_grad
    assert torch.equal(s, cc.score(xd))                                       # the score's own bits
    _within_stock("dx", dx.cpu(), g64, g32)
    half = torch.tensor([0.5], device=DEV)
    s_h, dx_h = cc.score_grad(xd, gscale=half)
    assert torch.equal(s_h, s) and torch.equal(dx_h, dx * 0.5)                # exactly half
    xa = xd.clone().requires_grad_(True)
    sf = cc.score_fixed(xa)
    assert torch.equal(sf.detach(), s) and sf.requires_grad
    sf.sum().backward()
    assert torch.equal(xa.grad, dx)                                           # the same dx bit for bit
    si, dxi = cc.score_grad(interleave(xd), interleaved=True)
    assert torch.equal(si, s) and torch.equal(reference_channel_order(dxi), dx)
    with pytest.raises(ValueError, match="601"):
        cc.score_grad(xd[:, :, :600])
    with pytest.raises(ValueError, match="cuda"):
        cc.score_grad(x)
    with pytest.raises(ValueError, match="gscale"):
        cc.score_grad(xd, gscale=torch.ones(2, device=DEV))
    plain = D.commit()
    assert not plain.has_grad
    with pytest.raises(ValueError, match="grad=True"):
        plain.score_grad(xd)
    with pytest.raises(ValueError, match="grad=True"):
        plain.score_fixed(xd)
    plain.close()
    cc.close()
    with pytest.raises(ValueError, match="closed"):
        cc.score_grad(xd)


@pytest.fixture(scope="module")
def separator(sd_default):
    """The default model on the device with one 601-frame mixture and target (shared: the spectrum test and the training test)."""
    from speechseparation_amd import weights
    from speechseparation_amd.bsrnn import BSRNN
    n = 614400
    m = BSRNN()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd_default.items()})
    m = m.to(DEV)
    mix = torch.from_numpy(weights.synth_waveform(2, n, seed=31)).to(DEV)
    speech = torch.from_numpy(weights.synth_waveform(2, n, seed=32)).to(DEV)
    return m, mix, speech


def test_score_grad_on_the_models_spectrum(separator):
    """2050 channels, the model's real output (metrics.critic_input): dp1 is realistically tiny there.  The same rule - stock fp32
    autograd's error x 4 + 2^-23 against float64 autograd - and interleaved equals planar bit for bit."""
    from speechseparation_amd import metrics
    from speechseparation_amd.discriminator import reference_channel_order
    m, mix, _ = separator
    D, cc = critic(2050, seed=17)
    cc.recommit(D)
    with torch.no_grad():
        x = metrics.critic_input(m.eval(), mix).contiguous()
    assert tuple(x.shape) == (2, 2050, 601)
    s, dx = cc.score_grad(x)
    assert torch.equal(s, cc.score(x))
    g64, g32 = _chain_reference({k: v.detach().cpu() for k, v in D.state_dict().items()}, 2050, x.cpu())
    print("max |dx| = %.3e" % float(dx.abs().max()))
    _within_stock("dx at 2050 channels", dx.cpu(), g64, g32)
    si, dxi = cc.score_grad(interleave(x), interleaved=True)
    assert torch.equal(si, s) and torch.equal(reference_channel_order(dxi), dx)


# ------------------------------------------------------------------------------------------------ 4. reproducibility and the snapshot
def test_reproducible_and_a_snapshot():
    from speechseparation_amd.discriminator import Discriminator
    native, lib, ctx = _lib()
    D = Discriminator(66)
    D.load_state_dict(cr.synth_critic_state(66, seed=21), strict=True)
    D = D.to(DEV)
    torch.cuda.synchronize()
    before = lib.bsrnn_debug_counter(0)
    cc = D.commit(grad=True)
    assert lib.bsrnn_debug_counter(0) - before == 4                            # the object's three blocks and the dx image
    x = torch.randn((2, 66, 684), generator=_gen(6), device=DEV)
    s0, dx0 = cc.score_grad(x)
    native.check(lib.bsrnn_critic_enable_grad(cc._h, None))                    # idempotent
    with torch.no_grad():
        for p in D.parameters():
            p.mul_(-0.5)
    torch.cuda.synchronize()
    before = lib.bsrnn_debug_counter(0)
    s1, dx1 = cc.score_grad(x)
    assert lib.bsrnn_debug_counter(0) == before                                # a second call at a shape allocates nothing
    assert torch.equal(s1, s0) and torch.equal(dx1, dx0)                       # equal bits; the module's new weights do not reach the snapshot
    assert cc.recommit(D) is cc
    s2, dx2 = cc.score_grad(x)
    fresh = D.commit(grad=True)
    s3, dx3 = fresh.score_grad(x)
    assert torch.equal(s2, s3) and torch.equal(dx2, dx3) and not torch.equal(dx2, dx0)
    # the gradient enabled after the commit: the image is built from the snapshot
    late = D.commit()
    native.check(lib.bsrnn_critic_enable_grad(late._h, None))
    late.has_grad = True
    assert torch.equal(late.score_grad(x)[1], dx2)
    for c in (late, fresh, cc):
        c.close()


# ------------------------------------------------------------------------------------------------ 5. range
def _exact_chain(D, x, score, gscale=1.0):
    """dx of the exact chain through the library's exposed layer calls (the kernels the re-run launches), from the call's own score:
    the tail's gradient in the kernel's order of operations, then bsrnn_critic_conv_backward layer by layer."""
    convs = [m for m in D.layers if isinstance(m, torch.nn.Conv1d)]
    ws, bs = [c.weight.detach() for c in convs], [c.bias.detach() for c in convs]
    ys, h = [], x
    for l in range(4):
        h = conv_forward(h, ws[l], bs[l], l < 3)
        ys.append(h)
    C, T4 = x.shape[0], ys[3].shape[2]
    s = score.reshape(())
    lw = D.layers2[0].weight.detach().reshape(-1)
    dev = lambda v: torch.tensor(float(v), device=DEV)                         # noqa: E731  (tensor / tensor: a true division)
    gp = (((dev(gscale) * ((1.0 - s) * s)) * lw) / dev(C)) / dev(T4)
    dy = gp.reshape(1, -1, 1).expand(C, -1, T4).contiguous()
    for l in (3, 2, 1, 0):
        dy, _, _ = conv_backward(x if l == 0 else ys[l - 1], ws[l], ys[l], dy, l < 3)
    return dy


def test_range_guard_and_exact_rerun():
    from speechseparation_amd.discriminator import reference_channel_order
    native, lib, ctx = _lib()
    D, cc = critic(66)
    D.load_state_dict(cr.synth_critic_state(66, seed=5), strict=True)
    cc.recommit(D)
    w = D.layers[0].weight.detach().clone()
    x = torch.randn((2, 66, 604), generator=_gen(5), device=DEV)
    s_ok, dx_ok = cc.score_grad(x)
    assert not torch.equal(dx_ok, _exact_chain(D, x, s_ok))                    # (the fp16x2 path is the other path)
    x_hot = x.clone()
    x_hot[1, 3, 100] = 7e4
    assert lib.bsrnn_get_range_policy(ctx) == native.RANGE_EXACT
    s, dx = cc.score_grad(x_hot)                                               # rc 0, and the exact kernels' bits
    assert torch.equal(s, cc.score(x_hot)) and torch.equal(dx, _exact_chain(D, x_hot, s))
    si, dxi = cc.score_grad(interleave(x_hot), interleaved=True)               # (the exact chain: a planar copy in, a scatter out)
    assert torch.equal(si, s) and torch.equal(reference_channel_order(dxi), dx)
    s2, dx2 = cc.score_grad(x)                                                 # the guard is taken: the next call is fp16x2 again
    assert torch.equal(s2, s_ok) and torch.equal(dx2, dx_ok)
    native.check(lib.bsrnn_set_range_policy(ctx, native.RANGE_DEFERRED))
    try:
        cc.score_grad(x_hot)                                                   # asynchronous, rc 0
        rc = lib.bsrnn_sync(ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == ERANGE and "65504" in lib.bsrnn_last_error().decode()
        assert lib.bsrnn_sync(ctx, None) == 0                                  # reported once
    finally:
        native.check(lib.bsrnn_set_range_policy(ctx, native.RANGE_EXACT))
    # a weight beyond the fp16 range: that object runs the exact chain
    w_hot = w.clone()
    w_hot[5, 1, 2] = 7e4
    D, cc = set_first_layer(66, w_hot)
    s3, dx3 = cc.score_grad(x)
    assert torch.equal(dx3, _exact_chain(D, x, s3)) and bool(torch.isfinite(dx3).all())
    s4, dx4 = cc.score_grad(interleave(x), interleaved=True)
    assert torch.equal(s4, s3) and torch.equal(reference_channel_order(dx4), dx3)
    set_first_layer(66, w)


# ------------------------------------------------------------------------------------------------ 6. training
def test_adversarial_train_loss_with_a_committed_critic(separator):
    """One score_fixed call on the model's interleaved spectrum; the loss is the plain loss + the score bit for bit; the gradients are
    those of Discriminator.score_fixed (the exact kernels through autograd and the reorder copy) up to rounding: per parameter tensor
    max |g_cc - g_module| <= 1e-3 max |g_module - g_plain| - a plumbing condition, a wrong order or factor gives O(1)."""
    from speechseparation_amd import train
    m, mix, speech = separator
    D, cc = critic(2050, seed=17)
    cc.recommit(D)

    def grads(**kw):
        for p in list(m.parameters()) + list(D.parameters()):
            p.grad = None
        loss, _ = train.train_loss(m.train(), mix, speech, **kw)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    calls = []
    fixed_of = cc.score_fixed

    def recorded(x, interleaved=False):
        calls.append((tuple(x.shape), interleaved, fixed_of(x, interleaved=interleaved)))
        return calls[-1][2]
    cc.score_fixed = recorded
    try:
        l0, g0 = grads()
        l1, g1 = grads(discriminator=cc, adversarial=True)
    finally:
        del cc.score_fixed
    shape, inter, score = calls.pop()
    assert shape == (2, 2050, 601) and inter is True and not calls                 # the model's interleaved spectrum, one call
    assert torch.equal(l1, l0 + score.detach().reshape(())) and float(score.detach()) != 0.0
    assert set(g0) == set(g1) and any(not torch.equal(g0[k], g1[k]) for k in g0)
    _, g2 = grads(discriminator=D, adversarial=True)
    assert all(p.grad is None for p in D.parameters())
    worst = 0.0
    for k in g0:
        moved = float((g2[k] - g0[k]).abs().max())
        off = float((g1[k] - g2[k]).abs().max())
        if moved > 0:
            worst = max(worst, off / moved)
        assert off <= 1e-3 * moved, (k, off, moved)
    print("worst max|g_cc - g_module| / max|g_module - g_plain| over the parameter tensors: %.3e" % worst)
    plain = D.commit()
    try:
        with pytest.raises(ValueError, match="adversarial"):
            train.train_loss(m.train(), mix, speech, discriminator=plain, adversarial=True)
    finally:
        plain.close()


# ------------------------------------------------------------------------------------------------ 7. arguments
def test_argument_refusals():
    from speechseparation_amd import spec
    native, lib, ctx = _lib()
    nx, ndp = 2 * 66 * 601, 2 * 1024 * 196
    buf = torch.zeros(2 * nx + ndp + 4096, device=DEV)
    before = buf.clone()
    at = lambda n: ctypes.c_void_p(buf.data_ptr() + 4 * n)                     # noqa: E731
    x, dx, dp, out, gs = at(0), at(nx), at(2 * nx), at(2 * nx + ndp + 4), at(2 * nx + ndp + 8)
    null = ctypes.c_void_p()
    D, cc = critic(66)
    h = cc._h

    def refused(rc, code, word):
        msg = lib.bsrnn_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    def both(args_score, args_l1, code, word):
        refused(lib.bsrnn_critic_score_grad(*args_score), code, word)
        refused(lib.bsrnn_critic_layer1_dx(*args_l1), code, word)

    def on(hd, C=2, T=601, order=0):
        return (hd, x, C, T, order, gs, out, dx, None), (hd, dp, C, T, order, dx, None)

    both(*on(null), EARG, "null")
    refused(lib.bsrnn_critic_score_grad(h, null, 2, 601, 0, gs, out, dx, None), EARG, "null")
    refused(lib.bsrnn_critic_score_grad(h, x, 2, 601, 0, gs, null, dx, None), EARG, "null")
    refused(lib.bsrnn_critic_score_grad(h, x, 2, 601, 0, gs, out, null, None), EARG, "null")
    refused(lib.bsrnn_critic_layer1_dx(h, null, 2, 601, 0, dx, None), EARG, "null")
    refused(lib.bsrnn_critic_layer1_dx(h, dp, 2, 601, 0, null, None), EARG, "null")
    both(*on(h, C=0), EARG, "C = 0")
    both(*on(h, T=600), EARG, "600")
    both(*on(h, order=2), EARG, "x_order")
    both(*on(h, order=-1), EARG, "x_order")
    both(*on(h, C=1 << 20), EARG, "2^31")
    both(*on(h, T=1 << 30), EARG, "2^31")
    refused(lib.bsrnn_critic_score_grad(h, x, 2, 601, 0, gs, out, at(nx - 1), None), EARG, "dx_dev overlaps x_dev")
    refused(lib.bsrnn_critic_score_grad(h, x, 2, 601, 0, gs, at(nx + 7), dx, None), EARG, "dx_dev overlaps score_dev")
    refused(lib.bsrnn_critic_score_grad(h, x, 2, 601, 0, gs, at(100), dx, None), EARG, "score_dev overlaps x_dev")
    refused(lib.bsrnn_critic_score_grad(h, x, 2, 601, 0, at(nx + 9), out, dx, None), EARG, "gscale_dev overlaps")
    refused(lib.bsrnn_critic_layer1_dx(h, dp, 2, 601, 0, at(2 * nx - 1), None), EARG, "dx_dev overlaps dp_dev")
    lay = (ctypes.c_int64 * 8)()
    refused(lib.bsrnn_critic_grad_layout(66, 2, 600, lay), EARG, "600")
    refused(lib.bsrnn_critic_grad_layout(66, 2, 601, None), EARG, "layout")
    refused(lib.bsrnn_critic_grad_layout(0, 2, 601, lay), EARG, "in_channels")
    assert lib.bsrnn_critic_grad_layout(66, 2, 601, lay) == 0 and list(lay)[:5] == [9, 2, 8, 369, 128]
    refused(lib.bsrnn_critic_enable_grad(null, None), EARG, "null")
    # an odd channel count has no interleaved form; before the first commit; committed but without the gradient
    odd = ctypes.c_void_p()
    native.check(lib.bsrnn_critic_create(ctx, 67, ctypes.byref(odd)))
    try:
        both(*on(odd, C=1, order=1), EARG, "odd")
        both(*on(odd, C=1), ESTATE, "commit")
    finally:
        lib.bsrnn_critic_destroy(odd)
    plain = D.commit()
    try:
        both(*on(plain._h), ESTATE, "enable_grad")
    finally:
        plain.close()
    # a host-only context: sizes first, then BSRNN_ESTATE
    v = spec.generate_bandsplits()[0]
    host = ctypes.c_void_p()
    native.check(lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(host)))
    hk = ctypes.c_void_p()
    try:
        native.check(lib.bsrnn_critic_create(host, 66, ctypes.byref(hk)))
        both(*on(hk, T=600), EARG, "600")
        both(*on(hk, order=2), EARG, "x_order")
        both(*on(hk, C=0), EARG, "C = 0")
        both(*on(hk, C=1 << 20), EARG, "2^31")
        refused(lib.bsrnn_critic_score_grad(hk, x, 2, 601, 0, gs, out, at(nx - 1), None), EARG, "dx_dev overlaps x_dev")
        both(*on(hk), ESTATE, "host-only")
        refused(lib.bsrnn_critic_enable_grad(hk, None), ESTATE, "host-only")
    finally:
        lib.bsrnn_critic_destroy(hk)
        lib.bsrnn_destroy(host)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                            # nothing was launched
    xs = torch.randn((2, 66, 601), generator=_gen(9), device=DEV)
    cc.recommit(D)
    s, g = cc.score_grad(xs)
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(g).all())     # the object is untouched by the refusals
