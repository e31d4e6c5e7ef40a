"""GPU: the critic (speechseparation_amd/discriminator.py, csrc/critic.hip) against the float64 restatement of tests/critic_reference.py:
the layer's forward and backward exactly on integer data and within the fp32 dot-product bound on normal variates, reproducibility, the
argument checks, the module, three optimizer steps, train_infer / train_loss with a critic and the train-discriminator.py entry point."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
import critic_reference as cr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from speechseparation_amd import _native, train
    return _native, _native.lib, train._context(torch.device(DEV))


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()


def conv_forward(x, w, b, leaky):
    native, lib, ctx = _lib()
    C, I, T = x.shape
    O = w.shape[0]
    y = torch.full((C, O, cr.t_out(T)), float("nan"), device=DEV)
    native.check(lib.bsrnn_critic_conv_forward(ctx, _p(x), _p(w), _p(b), _p(y), C, I, T, O, int(leaky), None))
    return y


def conv_backward(x, w, y, dy, leaky, want_dx=True):
    native, lib, ctx = _lib()
    C, I, T = x.shape
    O = w.shape[0]
    nan = float("nan")
    dx = torch.full((C, I, T), nan, device=DEV) if want_dx else None
    dw, db = torch.full((O, I, 16), nan, device=DEV), torch.full((O,), nan, device=DEV)
    native.check(lib.bsrnn_critic_conv_backward(ctx, _p(x), _p(w), _p(y), _p(dy), _p(dx), _p(dw), _p(db), C, I, T, O, int(leaky), None))
    return dx, dw, db


def ints(rng, shape):
    return torch.from_numpy(rng.integers(-2, 3, shape).astype(np.float32))


def slab_shape():
    """An I with at least three K slabs and a partial last one at O = 72, T = 211 (C = 2), read from the library's layout."""
    from speechseparation_amd.discriminator import conv_layout
    for I in range(17, 200):
        g = conv_layout(2, I, 211, 72)
        if g["slabs"] >= 3 and I % g["ch_per_slab"] != 0:
            return I, g
    raise AssertionError("no such I below 200")


# ------------------------------------------------------------------------------------------------ 1. indexing, exact
EXACT = [(1, 1, 16), (3, 5, 18), (66, 40, 19), (66, 40, 601), ("slabs", 72, 211), (4098, 1024, 19)]


@pytest.mark.parametrize("shape", EXACT, ids=lambda s: "%s-%d-%d" % s)
def test_integers_are_exact(shape):
    """Integers in [-2, 2]: every product and partial sum is an integer below 2^24 (16 I 4 + 2 < 2^24 up to I = 4098; the backward's sums
    have at most C T_out 4 resp. 6 O 4 terms), so pre-activations, dW, db and dx equal float64 whatever the order of additions.  The
    leaky forward is fl32(0.01f * v) of the exact pre-activation; exact zeros of it are common and check the slope-at-zero convention.
    The backward's sums are exact only while dp holds integers, so the full backward runs with the identity; under LeakyReLU
    dp = fl32(0.01f * dy) is no integer, and the convention is checked with one-hot dy at a positive, a zero and a negative output, where
    every gradient element is a single product."""
    I, O, T = shape
    if I == "slabs":
        I, g = slab_shape()
        print("slab case: I = %d, layout %s" % (I, g))
    C = 2
    rng = np.random.default_rng(7)
    x, w, b = ints(rng, (C, I, T)), ints(rng, (O, I, 16)), ints(rng, (O,))
    b[0] = -float((x[0, :, :16] * w[0]).sum())                                 # (an integer) y[0, 0, 0] is an exact zero at every shape
    To = cr.t_out(T)
    dy = ints(rng, (C, O, To))
    ref = cr.layer(x, w, b, dy, leaky=False)
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    assert float(ref["S_y"].max()) < 2 ** 24
    y_lin = conv_forward(xd, wd, bd, False)
    assert torch.equal(y_lin.cpu().double(), ref["pre"])
    y_leaky = conv_forward(xd, wd, bd, True)
    assert torch.equal(y_leaky.cpu().double(), cr.leaky32(ref["pre"]))
    print("zeros of the pre-activation: %d of %d" % (int((ref["pre"] == 0).sum()), ref["pre"].numel()))
    dx, dw, db = conv_backward(xd, wd, None, dyd, False)
    assert torch.equal(db.cpu().double(), ref["db"])
    assert torch.equal(dw, ref["dw"].to(torch.float32).to(DEV))              # (268 MB at full width: compared on the device)
    assert torch.equal(dx.cpu().double(), ref["dx"])                          # NaN pre-fill: the frames no window reaches are written zeros
    if T > 3 * (To - 1) + 16:
        assert float(dx[:, :, 3 * (To - 1) + 16:].abs().max()) == 0.0
    _, dw2, db2 = conv_backward(xd, wd, None, dyd, False, want_dx=False)      # a null dx skips that product and nothing else
    assert torch.equal(dw2, dw) and torch.equal(db2, db)
    if I * O * To > 66 * 40 * 2:
        return                                                               # the one-hot cases at the small shapes
    pre = ref["pre"]
    picks = [m.nonzero()[0] for m in (pre > 0, pre == 0, pre < 0) if bool(m.any())]         # (pre == 0 holds at [0, 0, 0] at least)
    assert float(pre[0, 0, 0]) == 0.0
    for c, o, t in (tuple(int(v) for v in p) for p in picks):
        hot = torch.zeros((C, O, To))
        hot[c, o, t] = 2.0
        r1 = cr.layer(x, w, b, hot, leaky=True)
        dx1, dw1, db1 = conv_backward(xd, wd, y_leaky, hot.to(DEV), True)
        slope = 1.0 if float(pre[c, o, t]) > 0 else float(np.float32(0.01))
        assert float(r1["dp"][c, o, t]) == 2.0 * slope
        assert torch.equal(db1.cpu().double(), r1["db"]) and torch.equal(dw1.cpu().double(), r1["dw"])
        assert torch.equal(dx1.cpu().double(), r1["dx"])


# ------------------------------------------------------------------------------------------------ 2. rounding
@pytest.mark.parametrize("shape", [(66, 40, 601), (1024, 128, 196)], ids=lambda s: "%d-%d-%d" % s)
def test_normal_variates_within_the_dot_product_bound(shape):
    """Every element of y, dW, db and dx within (n + 2) 2^-24 S of float64: n its number of products, S the same sum over absolute values
    (plus |b|).  The backward is given the restatement's y (rounded to fp32), so that both sides read the same signs."""
    I, O, T = shape
    C = 2
    rng = np.random.default_rng(11)
    x, w, b = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((C, I, T), (O, I, 16), (O,)))
    dy = torch.from_numpy(rng.standard_normal((C, O, cr.t_out(T))).astype(np.float32))
    xd, wd, bd, dyd = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
    for leaky in (False, True):
        ref = cr.layer(x, w, b, dy, leaky=leaky)
        y = conv_forward(xd, wd, bd, leaky).cpu().double()
        y32 = ref["y"].to(torch.float32)
        dx, dw, db = (t.cpu().double() for t in conv_backward(xd, wd, y32.to(DEV), dyd, leaky))
        for name, got, n in (("y", y, ref["n_y"]), ("dw", dw, ref["n_dw"]), ("db", db, ref["n_db"]), ("dx", dx, ref["n_dx"])):
            lim = cr.bound(n, ref["S_" + name])
            err = (got - ref[name]).abs()
            ratio = float((err / lim.clamp_min(1e-300)).max())
            print("%s leaky=%d: worst error / bound = %.3f" % (name, leaky, ratio))
            assert bool((err <= lim).all()), (name, leaky, ratio)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
def test_bit_reproducible():
    rng = np.random.default_rng(3)
    C, I, O, T = 2, 66, 40, 601
    x, w, b = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV) for s in ((C, I, T), (O, I, 16), (O,)))
    dy = torch.from_numpy(rng.standard_normal((C, O, cr.t_out(T))).astype(np.float32)).to(DEV)
    runs = []
    for _ in range(2):
        y = conv_forward(x, w, b, True)
        runs.append((y,) + conv_backward(x, w, y, dy, True))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_argument_errors():
    from speechseparation_amd import spec
    native, lib, ctx = _lib()
    EARG, ESTATE = 1, 2                                                        # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
    buf = torch.zeros(4096, device=DEV)
    before = buf.clone()
    p = _p(buf)

    def refused(rc, code, word):
        msg = lib.bsrnn_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    refused(lib.bsrnn_critic_conv_forward(ctx, p, p, p, p, 2, 3, 15, 5, 0, None), EARG, "15")
    refused(lib.bsrnn_critic_conv_backward(ctx, p, p, p, p, p, p, p, 2, 3, 15, 5, 0, None), EARG, "15")
    refused(lib.bsrnn_critic_conv_forward(ctx, p, p, p, p, 0, 3, 16, 5, 0, None), EARG, "C = 0")
    refused(lib.bsrnn_critic_conv_forward(ctx, p, p, p, p, 2, 1 << 20, 1 << 20, 5, 0, None), EARG, "2^31")
    null = ctypes.c_void_p()
    refused(lib.bsrnn_critic_conv_forward(ctx, p, null, p, p, 2, 3, 16, 5, 0, None), EARG, "null")
    refused(lib.bsrnn_critic_conv_forward(null, p, p, p, p, 2, 3, 16, 5, 0, None), EARG, "null")
    refused(lib.bsrnn_critic_conv_backward(ctx, p, p, p, p, p, null, p, 2, 3, 16, 5, 0, None), EARG, "null")
    refused(lib.bsrnn_critic_conv_backward(ctx, p, p, null, p, p, p, p, 2, 3, 16, 5, 1, None), EARG, "null")       # y is read when leaky
    out = (ctypes.c_int32 * 5)()
    refused(lib.bsrnn_critic_conv_layout(2, 3, 15, 5, out), EARG, "15")
    refused(lib.bsrnn_critic_conv_layout(2, 3, 16, 5, None), EARG, "layout")
    v = spec.generate_bandsplits()[0]
    host = ctypes.c_void_p()
    native.check(lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(host)))
    try:
        refused(lib.bsrnn_critic_conv_forward(host, p, p, p, p, 2, 3, 15, 5, 0, None), EARG, "15")                    # sizes before the device
        refused(lib.bsrnn_critic_conv_forward(host, p, p, p, p, 2, 3, 16, 5, 0, None), ESTATE, "host-only")
        refused(lib.bsrnn_critic_conv_backward(host, p, p, p, p, p, p, p, 2, 3, 16, 5, 0, None), ESTATE, "host-only")
    finally:
        lib.bsrnn_destroy(host)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                            # nothing was launched


# ------------------------------------------------------------------------------------------------ 5. the module
def _rel(a, ref):
    return float((a.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _within_stock(name, got, ref64, stock32):
    """max|a - ref64| / max|ref64| of the device at most 4 x stock fp32's, plus one fp32 ulp of max|ref64| (relative: 2^-23)."""
    e_dev, e_cpu = _rel(got, ref64), _rel(stock32, ref64)
    print("%-18s device %.3e   stock fp32 %.3e" % (name, e_dev, e_cpu))
    assert e_dev <= 4 * e_cpu + 2.0 ** -23, (name, e_dev, e_cpu)


@pytest.mark.parametrize("T", [601, 684])
def test_module_against_float64_and_stock_fp32(T):
    from speechseparation_amd.discriminator import Discriminator
    sd = cr.synth_critic_state(66, seed=5)
    ref64, ref32 = cr.CriticF64(66), cr.CriticF64(66, dtype=torch.float32)
    ref64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    ref32.load_state_dict(sd, strict=True)
    D = Discriminator(66)
    D.load_state_dict(ref64.state_dict(), strict=True)                       # strict both ways
    ref64.load_state_dict(D.state_dict(), strict=True)
    D = D.to(DEV)
    x = torch.from_numpy(np.random.default_rng(T).standard_normal((2, 66, T)).astype(np.float32))
    s64, s32 = ref64(x.double()), ref32(x)
    s64.sum().backward()
    s32.sum().backward()
    s = D(x.to(DEV))
    assert tuple(s.shape) == (1,)
    s.sum().backward()
    _within_stock("score", s.detach().cpu(), s64.detach(), s32.detach())
    g64, g32 = dict(ref64.named_parameters()), dict(ref32.named_parameters())
    for k, p in D.named_parameters():
        _within_stock(k, p.grad.cpu(), g64[k].grad, g32[k].grad)
    with pytest.raises(ValueError, match="601"):
        D(x[:, :, :600].to(DEV))
    with pytest.raises(ValueError, match="cuda"):
        D(x)


# ------------------------------------------------------------------------------------------------ 6. three optimizer steps
def test_three_critic_steps_follow_torch_adam():
    """The loop's loss score_speech + (1 - score_orig) under the project's AdamW(lr 1e-4, weight_decay 0) against float64 torch.optim.Adam;
    the tolerances of test_three_train_steps_follow_torch_adamw."""
    from speechseparation_amd import train
    from speechseparation_amd.discriminator import Discriminator
    sd = cr.synth_critic_state(66, seed=9)
    ref = cr.CriticF64(66)
    ref.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    D = Discriminator(66)
    D.load_state_dict(sd, strict=True)
    D = D.to(DEV)
    rng = np.random.default_rng(13)
    a, b = (torch.from_numpy(rng.standard_normal((2, 66, 601)).astype(np.float32)) for _ in range(2))
    opt_ref = torch.optim.Adam(ref.parameters(), lr=1e-4)
    opt = train.AdamW(D.parameters(), lr=1e-4, weight_decay=0)
    losses, ref_losses = [], []
    for _ in range(3):
        lr_ = ref(a.double()) + (1 - ref(b.double()))
        lr_.sum().backward()
        opt_ref.step()
        opt_ref.zero_grad()
        ref_losses.append(float(lr_.detach()))
        l = D(a.to(DEV)) + (1 - D(b.to(DEV)))
        l.sum().backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(l.detach()))
    print("losses", losses, "reference", ref_losses)
    for u, v in zip(losses, ref_losses):
        assert abs(u - v) < 2e-4 * abs(v)
    rp = dict(ref.named_parameters())
    worst = max((float((p.detach().cpu().double() - rp[k].detach()).abs().max()), k) for k, p in D.named_parameters())
    print("largest parameter difference after three steps: %.2e (%s)" % worst)
    assert worst[0] < 2e-3


# ------------------------------------------------------------------------------------------------ 7. train_infer / train_loss with a critic
def test_train_infer_and_train_loss_with_a_critic(sd_default):
    from speechseparation_amd import metrics, train, weights
    from speechseparation_amd.bsrnn import BSRNN, Discriminator
    n = 614400
    m = BSRNN()
    m.load_state_dict({k: torch.from_numpy(np.array(a, copy=True)) for k, a in sd_default.items()})
    m = m.to(DEV)
    csd = cr.synth_critic_state(2050, seed=17)
    D = Discriminator(2050)
    D.load_state_dict(csd, strict=True)
    D = D.to(DEV)
    ref64, ref32 = cr.CriticF64(2050), cr.CriticF64(2050, dtype=torch.float32)
    ref64.load_state_dict({k: v.double() for k, v in csd.items()}, strict=True)
    ref32.load_state_dict(csd, strict=True)
    mix = torch.from_numpy(weights.synth_waveform(2, n, seed=31)).to(DEV)
    speech = torch.from_numpy(weights.synth_waveform(2, n, seed=32)).to(DEV)
    sample = (mix.unsqueeze(0), speech.unsqueeze(0))
    base = metrics.train_infer(m.eval(), None, sample)
    got = metrics.train_infer(m, D, sample)
    for a, b in zip(got[1:], base[1:]):
        assert a.dim() == 0 and float(a) == float(b)                          # sdr, sdr2, sdr3 bit for bit
    x2 = metrics.critic_input(m, mix).cpu()                                   # the model's output in the reference's channel order
    assert tuple(x2.shape) == (2, 2050, 601)
    with torch.no_grad():
        s64, s32 = ref64(x2.double()), ref32(x2)
    diff = torch.tensor([float(got[0]) - float(base[0])], dtype=torch.float64)
    _within_stock("loss - loss_None", diff, s64, s32)
    short = (mix[:, :n - 1024].unsqueeze(0), speech[:, :n - 1024].unsqueeze(0))
    with pytest.raises(ValueError, match="601"):
        metrics.train_infer(m, D, short)

    def grads(**kw):
        for p in list(m.parameters()) + list(D.parameters()):
            p.grad = None
        loss, _ = train.train_loss(m.train(), mix, speech, **kw)
        loss.backward()
        return float(loss), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    l0, g0 = grads()
    l1, g1 = grads(discriminator=D)
    assert all(p.grad is None for p in D.parameters())
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)  # the score is a constant: gradients bit for bit
    assert l1 != l0
    l2, g2 = grads(discriminator=D, adversarial=True)
    assert all(p.grad is None for p in D.parameters())                        # the critic is held fixed
    assert any(not torch.equal(g0[k], g2[k]) for k in g0)
    # dx of the first layer (through all four) against float64 autograd on the same input
    xin = x2.clone()
    for p in list(ref64.parameters()) + list(ref32.parameters()):
        p.requires_grad_(False)
    x64 = xin.double().requires_grad_(True)
    x32 = xin.clone().requires_grad_(True)
    ref64(x64).sum().backward()
    ref32(x32).sum().backward()
    xd = xin.to(DEV).requires_grad_(True)
    D.score_fixed(xd).sum().backward()
    _within_stock("dx of layer 0", xd.grad.cpu(), x64.grad, x32.grad)


# ------------------------------------------------------------------------------------------------ 8. the entry point
def test_train_discriminator_entry_point(tmp_path):
    script = os.path.join(REPO, "train-discriminator.py")
    out = subprocess.run([sys.executable, script, "--synthetic", "2", "--mini", "--epochs", "1"], cwd=str(tmp_path), capture_output=True,
                         text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "Epoch 0 Loss" in out.stdout and "Validation Loss" in out.stdout
    sd = torch.load(str(tmp_path / "discriminator.pth"), map_location="cpu", weights_only=True)
    ref = cr.CriticF64(2050)
    ref.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
