"""GPU: the committed critic (Discriminator.commit() -> CommittedCritic; bsrnn_critic_create / _commit / _score; csrc/critic_score.hip):
the fp16x2 first layer exactly on integer data and within the three-term bound on normal variates, the score by the module's rule, both
input orders, the range guard and its exact re-run, the snapshot, the training entry points and the argument refusals."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import critic_reference as cr
from test_gpu_critic import _within_stock, conv_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EARG, ESTATE, ERANGE = 1, 2, 6                                                 # BSRNN_* of include/bsrnn_hip.h
_modules = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_critics():
    """The shared modules and their committed critics (about 1.2 GB of device memory at 4098 and 2050 channels) go with this file."""
    yield
    for _, cc in _modules.values():
        cc.close()
    _modules.clear()
    torch.cuda.empty_cache()


def _lib():
    from speechseparation_amd import _native, train
    return _native, _native.lib, train._context(torch.device(DEV))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()


def critic(I, seed=5):
    """One Discriminator(I) on the device with synthetic weights and its CommittedCritic, shared by the tests (a test that changes the
    weights recommits; every test that reads y1 commits its own first layer first)."""
    from speechseparation_amd.discriminator import Discriminator
    if I not in _modules:
        D = Discriminator(I)
        if I <= 2050:
            D.load_state_dict(cr.synth_critic_state(I, seed=seed), strict=True)
        D = D.to(DEV)
        _modules[I] = (D, D.commit())
    return _modules[I]


def set_first_layer(I, w, b):
    D, cc = critic(I)
    with torch.no_grad():
        D.layers[0].weight.copy_(w)
        D.layers[0].bias.copy_(b)
    cc.recommit(D)
    return D, cc


def interleave(x):
    """The inverse of reference_channel_order: planar [C, 2 F, T] -> (re, im, re, im, ...)."""
    Fb = x.shape[1] // 2
    return torch.stack((x[:, :Fb], x[:, Fb:]), dim=2).reshape(x.shape).contiguous()


def ints(gen, shape):
    return torch.randint(-2, 3, shape, generator=gen, device=DEV).float()


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------ 1. integers
@pytest.mark.parametrize("I", [2, 7, 10, 66])
def test_integers_are_exact(I):
    """Integers in [-2, 2] are fp16 values, so every second piece is zero, every product and partial sum an integer below 2^24: y1
    equals float64 whatever the order of the additions - over partial channel stages (I = 7), partial frame tiles (196, 197 and 260
    frames in tiles of 128), one slab (2, 7, 10 channels) and seven slabs with a partial last one (66)."""
    from speechseparation_amd.discriminator import reference_channel_order
    g = _gen(I)
    w, b = ints(g, (1024, I, 16)), ints(g, (1024,))
    _, cc = set_first_layer(I, w, b)
    for T in (601, 604, 793):
        for C in (1, 3):
            x = ints(g, (C, I, T))
            ref = cr.leaky32(F.conv1d(x.cpu().double(), w.cpu().double(), b.cpu().double(), stride=3))
            _, y1 = cc.score(x, return_y1=True)
            assert tuple(y1.shape) == (C, 1024, cr.t_out(T))
            assert torch.equal(y1.cpu().double(), ref), (I, T, C)
            if I % 2 == 0:
                _, y1i = cc.score(interleave(x), interleaved=True, return_y1=True)
                assert torch.equal(reference_channel_order(interleave(x)), x) and torch.equal(y1i, y1), (I, T, C)


def test_integers_at_full_width_equal_the_exact_kernel():
    """4098 channels, 601 frames, 2 rows - the only shape with the full K-slab count: y1 equals bsrnn_critic_conv_forward's bit for
    bit (both exact: 16 * 4098 * 4 + 2 < 2^24), compared on the device."""
    from speechseparation_amd.discriminator import score_layout
    g = _gen(4098)
    w, b, x = ints(g, (1024, 4098, 16)), ints(g, (1024,)), ints(g, (2, 4098, 601))
    _, cc = set_first_layer(4098, w, b)
    lay = score_layout(4098, 2, 601)
    print("layout", lay)
    assert lay["slabs"] >= 16 and 4098 % lay["ch_per_slab"] != 0
    _, y1 = cc.score(x, return_y1=True)
    want = conv_forward(x, w, b, True)
    assert torch.equal(y1, want)
    _, y1i = cc.score(interleave(x), interleaved=True, return_y1=True)
    assert torch.equal(y1i, want)


# ------------------------------------------------------------------------------------------------ 2. rounding
def test_normal_variates_within_the_three_term_bound():
    """Every element of y1 within (n + 14) 2^-24 S of float64, n = 16 I products, S = sum |w| |x| + |b|: (n + 2) u S is the fp32 dot
    product's bound in any order (critic_reference.bound); the 12 u S more is the operands' representation - a ~ a1 + 2^-11 a2 keeps
    22 bits, 2^-22 relative per operand, and the dropped a2 b2 2^-22 is at most 2^-22 |a b|: 3 x 2^-22 = 12 u per product (derived in
    tests/test_critic_score_reference.py, which holds the scheme itself to the same bound).  Both input orders."""
    for I, T in ((66, 601), (10, 793)):
        rng = np.random.default_rng(11 + I)
        x, w, b = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((2, I, T), (1024, I, 16), (1024,)))
        ref = cr.layer(x, w, b, torch.zeros(2, 1024, cr.t_out(T)), leaky=True, want_dx=False)
        lim = (16 * I + 14) * cr.U * ref["S_y"]
        _, cc = set_first_layer(I, w.to(DEV), b.to(DEV))
        for name, xin, inter in (("planar", x.to(DEV), False), ("interleaved", interleave(x.to(DEV)), True)):
            _, y1 = cc.score(xin, interleaved=inter, return_y1=True)
            err = (y1.cpu().double() - ref["y"]).abs()
            print("I = %d, T = %d, %s: worst error / bound = %.3f" % (I, T, name, float((err / lim).max())))
            assert bool((err <= lim).all())


def test_normal_variates_at_full_width_against_the_exact_kernel():
    """4098 channels (weights at torch's scale, uniform +-0.0039): y1 within the sum of both bounds of the exact kernel's,
    (n + 2) u S + (n + 14) u S, S from the exact kernel on |x|, |W|, |b| (all positive: the activation is the identity there)."""
    g = _gen(8)
    k = 1.0 / np.sqrt(4098 * 16)
    w = (torch.rand((1024, 4098, 16), generator=g, device=DEV) * 2 - 1) * k
    b = (torch.rand((1024,), generator=g, device=DEV) * 2 - 1) * k
    x = torch.randn((2, 4098, 601), generator=g, device=DEV)
    _, cc = set_first_layer(4098, w, b)
    _, y1 = cc.score(x, return_y1=True)
    exact = conv_forward(x, w, b, True)
    S = conv_forward(x.abs(), w.abs(), b.abs(), True).double()
    n = 16 * 4098
    lim = (2 * n + 16) * cr.U * S
    err = (y1.double() - exact.double()).abs()
    print("4098 channels: worst |fp16x2 - exact| / ((2 n + 16) u S) = %.4f" % float((err / lim).max()))
    assert bool((err <= lim).all())
    assert not torch.equal(y1, exact)                                          # (it is the other path)


# ------------------------------------------------------------------------------------------------ 3. the score
@pytest.mark.parametrize("T", [601, 684])
def test_score_against_float64_and_stock_fp32(T):
    from speechseparation_amd.discriminator import Discriminator
    sd = cr.synth_critic_state(66, seed=5)
    ref64, ref32 = cr.CriticF64(66), cr.CriticF64(66, dtype=torch.float32)
    ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ref32.load_state_dict(sd, strict=True)
    D = Discriminator(66)
    D.load_state_dict(sd, strict=True)
    cc = D.to(DEV).commit()
    x = torch.from_numpy(np.random.default_rng(T).standard_normal((2, 66, T)).astype(np.float32))
    with torch.no_grad():
        s64, s32 = ref64(x.double()), ref32(x)
    s = cc.score(x.to(DEV))
    assert tuple(s.shape) == (1,) and not s.requires_grad
    _within_stock("score", s.cpu(), s64, s32)
    _within_stock("score, interleaved", cc.score(interleave(x.to(DEV)), interleaved=True).cpu(), s64, s32)
    with pytest.raises(ValueError, match="601"):
        cc.score(x[:, :, :600].to(DEV))
    with pytest.raises(ValueError, match="cuda"):
        cc.score(x)
    cc.close()
    cc.close()
    with pytest.raises(ValueError, match="closed"):
        cc.score(x.to(DEV))


# ------------------------------------------------------------------------------------------------ 4. input order
def test_interleaved_equals_planar_bit_for_bit():
    from speechseparation_amd.discriminator import reference_channel_order
    D, cc = critic(66)
    cc.recommit(D)
    y = torch.randn((3, 66, 793), generator=_gen(4), device=DEV)               # an interleaved spectrum
    s_i, y1_i = cc.score(y, interleaved=True, return_y1=True)
    s_p, y1_p = cc.score(reference_channel_order(y), return_y1=True)
    assert torch.equal(s_i, s_p) and torch.equal(y1_i, y1_p)
    assert not torch.equal(cc.score(y), s_i)                                   # (the order matters)


# ------------------------------------------------------------------------------------------------ 5. range
def test_range_guard_and_exact_rerun():
    native, lib, ctx = _lib()
    D, cc = critic(66)
    cc.recommit(D)
    w, b = D.layers[0].weight.detach(), D.layers[0].bias.detach()
    x = torch.randn((2, 66, 604), generator=_gen(5), device=DEV)
    s_ok, y1_ok = cc.score(x, return_y1=True)
    x_hot = x.clone()
    x_hot[1, 3, 100] = 7e4
    assert lib.bsrnn_get_range_policy(ctx) == native.RANGE_EXACT
    s, y1 = cc.score(x_hot, return_y1=True)                                    # rc 0 (score raises otherwise), and the exact kernels' bits
    assert torch.equal(y1, conv_forward(x_hot, w, b, True))
    assert bool(torch.isfinite(s).all())
    s2, y1_2 = cc.score(x, return_y1=True)                                     # the guard is taken: the next call is fp16x2 again
    assert torch.equal(s2, s_ok) and torch.equal(y1_2, y1_ok) and not torch.equal(y1_ok, conv_forward(x, w, b, True))
    native.check(lib.bsrnn_set_range_policy(ctx, native.RANGE_DEFERRED))
    try:
        cc.score(x_hot)                                                        # asynchronous, rc 0
        rc = lib.bsrnn_sync(ctx, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == ERANGE and "65504" in lib.bsrnn_last_error().decode()
        assert lib.bsrnn_sync(ctx, None) == 0                                  # reported once
    finally:
        native.check(lib.bsrnn_set_range_policy(ctx, native.RANGE_EXACT))
    # a weight beyond the fp16 range: that handle scores on the exact kernels
    w_hot = w.clone()
    w_hot[5, 1, 2] = 7e4
    _, cc = set_first_layer(66, w_hot, b)
    s3, y1_3 = cc.score(x, return_y1=True)
    assert torch.equal(y1_3, conv_forward(x, w_hot, b, True)) and bool(torch.isfinite(s3).all())
    _, y1_4 = cc.score(interleave(x), interleaved=True, return_y1=True)        # (the exact kernels read a planar copy)
    assert torch.equal(y1_4, y1_3)
    set_first_layer(66, w, b)


# ------------------------------------------------------------------------------------------------ 6. snapshot
def test_commit_is_a_snapshot():
    from speechseparation_amd.discriminator import Discriminator
    native, lib, ctx = _lib()
    D = Discriminator(66)
    D.load_state_dict(cr.synth_critic_state(66, seed=21), strict=True)
    D = D.to(DEV)
    cc = D.commit()
    x = torch.randn((2, 66, 684), generator=_gen(6), device=DEV)
    s0 = cc.score(x)
    with torch.no_grad():
        for p in D.parameters():
            p.mul_(-0.5)
    torch.cuda.synchronize()
    before = lib.bsrnn_debug_counter(0)
    s1 = cc.score(x)
    assert lib.bsrnn_debug_counter(0) == before                                # a second score at a shape allocates nothing
    assert torch.equal(s1, s0)                                                 # the module's new weights do not reach the snapshot
    assert cc.recommit(D) is cc
    s2 = cc.score(x)
    fresh = D.commit()
    assert torch.equal(s2, fresh.score(x)) and not torch.equal(s2, s0)
    fresh.close()
    cc.close()
    with pytest.raises(ValueError, match="Discriminator"):
        critic(66)[1].recommit(Discriminator(10).to(DEV))


# ------------------------------------------------------------------------------------------------ 7. training
def test_train_loss_and_train_infer_with_a_committed_critic(sd_default):
    from speechseparation_amd import metrics, train, weights
    from speechseparation_amd.bsrnn import BSRNN
    n = 614400
    m = BSRNN()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd_default.items()})
    m = m.to(DEV)
    D, cc = critic(2050, seed=17)
    mix = torch.from_numpy(weights.synth_waveform(2, n, seed=31)).to(DEV)
    speech = torch.from_numpy(weights.synth_waveform(2, n, seed=32)).to(DEV)

    def grads(**kw):
        for p in m.parameters():
            p.grad = None
        loss, _ = train.train_loss(m.train(), mix, speech, **kw)
        loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    calls = []
    score_of = cc.score

    def recorded(x, interleaved=False):
        calls.append((tuple(x.shape), interleaved, score_of(x, interleaved=interleaved)))
        return calls[-1][2]
    cc.score = recorded
    try:
        l0, g0 = grads()
        l1, g1 = grads(discriminator=cc)
        shape, inter, score = calls.pop()
        assert shape == (2, 2050, 601) and inter is True and not calls             # the model's interleaved spectrum, one call
        assert torch.equal(l1, l0 + score.reshape(())) and float(score) != 0.0
        assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)  # a constant: the gradients bit for bit
        with pytest.raises(ValueError, match="adversarial"):
            train.train_loss(m.train(), mix, speech, discriminator=cc, adversarial=True)
        sample = (mix.unsqueeze(0), speech.unsqueeze(0))
        base = metrics.train_infer(m.eval(), None, sample)
        got = metrics.train_infer(m, cc, sample)
        shape, inter, s_eval = calls.pop()
        assert shape == (2, 2050, 601) and inter is True and not calls
    finally:
        del cc.score
    assert float(got[0]) == float(base[0] + s_eval.double().cpu().reshape(()))
    for a, b in zip(got[1:], base[1:]):
        assert float(a) == float(b)
    # and it is the critic's score: float64 and stock fp32 on the same input, by the module's rule
    x2 = metrics.critic_input(m, mix).cpu()
    ref64, ref32 = cr.CriticF64(2050), cr.CriticF64(2050, dtype=torch.float32)
    sd = {k: v.detach().cpu() for k, v in D.state_dict().items()}
    ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ref32.load_state_dict(sd, strict=True)
    with torch.no_grad():
        _within_stock("train_infer's score", s_eval.cpu(), ref64(x2.double()), ref32(x2))


# ------------------------------------------------------------------------------------------------ 8. arguments
def test_argument_refusals():
    from speechseparation_amd import spec
    native, lib, ctx = _lib()
    buf = torch.zeros(2 * 66 * 601 + 4096, device=DEV)
    before = buf.clone()
    p, far = _p(buf), ctypes.c_void_p(buf.data_ptr() + 4 * (2 * 66 * 601 + 8))
    out = ctypes.c_void_p(buf.data_ptr() + 4 * (2 * 66 * 601 + 4))
    null = ctypes.c_void_p()
    D, cc = critic(66)
    h = cc._h

    def refused(rc, code, word):
        msg = lib.bsrnn_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    refused(lib.bsrnn_critic_score(null, p, 2, 601, 0, out, null, None), EARG, "null")
    refused(lib.bsrnn_critic_score(h, null, 2, 601, 0, out, null, None), EARG, "null")
    refused(lib.bsrnn_critic_score(h, p, 2, 601, 0, null, null, None), EARG, "null")
    refused(lib.bsrnn_critic_score(h, p, 2, 600, 0, out, null, None), EARG, "600")
    refused(lib.bsrnn_critic_score(h, p, 0, 601, 0, out, null, None), EARG, "C = 0")
    refused(lib.bsrnn_critic_score(h, p, 2, 601, 2, out, null, None), EARG, "x_order")
    refused(lib.bsrnn_critic_score(h, p, 2, 601, -1, out, null, None), EARG, "x_order")
    refused(lib.bsrnn_critic_score(h, p, 1 << 20, 601, 0, out, null, None), EARG, "2^31")
    refused(lib.bsrnn_critic_score(h, p, 2, 1 << 30, 0, out, null, None), EARG, "2^31")
    refused(lib.bsrnn_critic_score(h, p, 2, 601, 0, ctypes.c_void_p(buf.data_ptr() + 4 * 100), null, None), EARG, "score_dev overlaps")
    refused(lib.bsrnn_critic_score(h, p, 2, 601, 0, far, ctypes.c_void_p(buf.data_ptr() + 4 * (2 * 66 * 601 - 1)), None), EARG, "y1_dev overlaps")
    lay = (ctypes.c_int64 * 10)()
    refused(lib.bsrnn_critic_score_layout(66, 2, 600, lay), EARG, "600")
    refused(lib.bsrnn_critic_score_layout(66, 2, 601, None), EARG, "layout")
    refused(lib.bsrnn_critic_score_layout(0, 2, 601, lay), EARG, "in_channels")
    assert lib.bsrnn_critic_score_layout(66, 2, 601, lay) == 0 and list(lay)[:4] == [196, 61, 16, 1]
    made = ctypes.c_void_p()
    refused(lib.bsrnn_critic_create(null, 66, ctypes.byref(made)), EARG, "null")
    refused(lib.bsrnn_critic_create(ctx, 0, ctypes.byref(made)), EARG, "in_channels")
    refused(lib.bsrnn_critic_create(ctx, 66, None), EARG, "nowhere")
    four = (ctypes.c_void_p * 4)(p, p, p, p)
    three = (ctypes.c_void_p * 4)(p, p, null, p)
    refused(lib.bsrnn_critic_commit(null, four, four, p, p, None), EARG, "null")
    refused(lib.bsrnn_critic_commit(h, three, four, p, p, None), EARG, "layer 2")
    refused(lib.bsrnn_critic_commit(h, four, four, null, p, None), EARG, "null")
    # an odd channel count has no interleaved form; a score before the first commit
    odd = ctypes.c_void_p()
    native.check(lib.bsrnn_critic_create(ctx, 67, ctypes.byref(odd)))
    try:
        refused(lib.bsrnn_critic_score(odd, p, 1, 601, 1, out, null, None), EARG, "odd")
        refused(lib.bsrnn_critic_score(odd, p, 1, 601, 0, out, null, None), ESTATE, "commit")
    finally:
        lib.bsrnn_critic_destroy(odd)
    # a host-only context: sizes first, then BSRNN_ESTATE
    v = spec.generate_bandsplits()[0]
    host = ctypes.c_void_p()
    native.check(lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(host)))
    hk = ctypes.c_void_p()
    try:
        native.check(lib.bsrnn_critic_create(host, 66, ctypes.byref(hk)))
        refused(lib.bsrnn_critic_score(hk, p, 2, 600, 0, out, null, None), EARG, "600")
        refused(lib.bsrnn_critic_score(hk, p, 2, 601, 2, out, null, None), EARG, "x_order")
        refused(lib.bsrnn_critic_score(hk, p, 2, 601, 0, out, null, None), ESTATE, "host-only")
        refused(lib.bsrnn_critic_commit(hk, four, four, p, p, None), ESTATE, "host-only")
    finally:
        lib.bsrnn_critic_destroy(hk)
        lib.bsrnn_destroy(host)
    lib.bsrnn_critic_destroy(None)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                            # nothing was launched
    x = torch.randn((2, 66, 601), generator=_gen(9), device=DEV)
    cc.recommit(D)
    assert bool(torch.isfinite(cc.score(x)).all())                             # the object is untouched by the refusals
