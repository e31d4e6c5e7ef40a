"""The reference's `Discriminator` (bsrnn.py:512-536) on the HIP library: the critic of `train-discriminator.py`.

Four `Conv1d(kernel 16, stride 3)` layers, `in_channels` -> 1024 -> 128 -> 64 -> 32, LeakyReLU after the first three, then the mean over
time, the mean over the rows, `Linear(32, 1)` and a sigmoid: [C, in_channels, T] -> [1].  Every convolution is a
`torch.autograd.Function` over `bsrnn_critic_conv_forward` / `bsrnn_critic_conv_backward` (exact fp32, bit-reproducible), the Linear
layer goes through `bsrnn_linear_train_*` (train.LinearFunction); the two means and the sigmoid are torch on the same device.  No CPU
fallback: the library has to be there and the tensors on the GPU.

`Discriminator.commit()` freezes the module into a `CommittedCritic`: the library's `bsrnn_critic` object, which scores in ONE call with
the first layer on the fp16x2 matrix path (fp32 in and out, range guard, exact re-run) and keeps its own copy of the weights - the
critic as a separator's training loop uses it, under no_grad.  `commit(grad=True)` gives that object its gradient as well:
`score_grad` returns the score and d score / d x from one call (`bsrnn_critic_score_grad`, the first layer's dx on the fp16x2 matrix
path, no dW anywhere), and `score_fixed` wraps it for autograd - the adversarial term of `train.train_loss`.
`score_ragged`, `score_grad_ragged` and `score_fixed_ragged` do the same for every clip of a padded batch in one call
(`bsrnn_critic_score_ragged` / `_score_grad_ragged`) - the critic term of `train.train_loss_ragged`.

`critic_spectrum` forms the critic's input as the reference's train-discriminator.py:62-68 does - the 4096-point analysis, real parts
then imaginary parts, 4098 channels - with the library's `bsrnn_critic_spectrum`.
"""
import ctypes

import torch
from torch import nn

from . import _native
from .train import LinearFunction, _context, _f32c, _p, _s

_lib = _native.lib

WIDTHS = (1024, 128, 64, 32)            # output channels of the four layers (CRITIC_WIDTHS of csrc/critic_host.h)
KERNEL, STRIDE = 16, 3
MIN_FRAMES = 601                        # the shortest input that reaches the last layer: 601 -> 196 -> 61 -> 16 -> 1


def frames_out(T):
    """Frames behind one layer: (T - 16) // 3 + 1 for T >= 16, else 0."""
    return (T - KERNEL) // STRIDE + 1 if T >= KERNEL else 0


def conv_layout(C, I, T, O):
    """bsrnn_critic_conv_layout as a dict: T_out, the forward's K slabs (count, input channels per slab) and the chunks of the dW / db
    reduction (count, frames per chunk)."""
    out = (ctypes.c_int32 * 5)()
    _native.check(_lib.bsrnn_critic_conv_layout(C, I, T, O, out))
    return dict(zip(("T_out", "slabs", "ch_per_slab", "dw_chunks", "dw_frames"), out))


def spectrum_layout(R, n):
    """bsrnn_critic_spectrum_layout as a dict: the frames T = 1 + n // 1024, the slabs a call of R rows x n samples runs in, the frames
    per slab and the workspace in floats (never more than 128 * 32 * 4098, whatever the clip)."""
    out = (ctypes.c_int64 * 4)()
    _native.check(_lib.bsrnn_critic_spectrum_layout(R, n, out))
    return dict(zip(("T", "slabs", "frames_per_slab", "scratch_floats"), out))


def critic_spectrum(wave, scale=1.0):
    """The critic's input of train-discriminator.py:62-68 on the library's kernel: wave [R, n] (cuda, n > 2048) ->
    torch.cat((X.real, X.imag), dim=1) of X = torch.stft(wave * scale, n_fft=4096, hop_length=1024, window=hann_window(4096)), i.e.
    [R, 4098, 1 + n // 1024] on the wave's device.  `scale` is applied to every sample before the window, as the product wave * scale
    rounds; no gradient (the critic's input is data).  No CPU fallback."""
    if not isinstance(wave, torch.Tensor) or wave.dim() != 2:
        raise ValueError("critic_spectrum: expected wave [R, n], got %s" % (tuple(getattr(wave, "shape", ())),))
    if not wave.is_cuda:
        raise ValueError("critic_spectrum: the transform runs on the GPU: wave must be a cuda tensor (there is no CPU fallback)")
    R, n = wave.shape
    dev = wave.device
    w = _f32c(wave)
    with torch.cuda.device(dev):
        x = torch.empty((R, 4098, 1 + n // 1024), device=dev)
        _native.check(_lib.bsrnn_critic_spectrum(_context(dev), _p(w), n, _p(x), R, n, float(scale), _s(dev)))
    return x


def reference_channel_order(y):
    """The library's interleaved spectrum [R, 2 F, T] (re, im, re, im, ...) in the order the reference feeds its critic:
    torch.cat((x.real, x.imag), dim=1) of m_dataset.py:205 - all real parts, then all imaginary parts."""
    return torch.cat((y[:, 0::2, :], y[:, 1::2, :]), dim=1)


def score_layout(in_channels, C, T):
    """bsrnn_critic_score_layout as a dict: the frames behind the four layers, the K slabs of the fp16x2 first layer, the workspace of
    a score in floats (and with the planar copy of an interleaved input on the exact kernels), the bytes of the fp16x2 image and of the
    fp32 snapshot a CommittedCritic holds."""
    out = (ctypes.c_int64 * 10)()
    _native.check(_lib.bsrnn_critic_score_layout(in_channels, C, T, out))
    v = list(out)
    return dict(frames=v[0:4], slabs=v[4], ch_per_slab=v[5], ws_floats=v[6], ws_exact_floats=v[7], image_bytes=v[8], snapshot_bytes=v[9])


def grad_layout(in_channels, C, T):
    """bsrnn_critic_grad_layout as a dict: the tiles of the fp16x2 dx (input channels, input positions per row) and a tile's extent,
    the workspace of a score with its gradient in floats (and with the exact chain's planar copies), the bytes of the dx image."""
    out = (ctypes.c_int64 * 8)()
    _native.check(_lib.bsrnn_critic_grad_layout(in_channels, C, T, out))
    v = list(out)
    return dict(i_tiles=v[0], s_tiles=v[1], tile_channels=v[2], tile_positions=v[3], tile_frames=v[4], ws_floats=v[5], ws_exact_floats=v[6],
                image_bytes=v[7])


class _CommittedScoreFunction(torch.autograd.Function):
    """score = cc(x) with the gradient kept from the same library call: backward returns dx * grad_output."""

    @staticmethod
    def forward(ctx, x, cc, interleaved):
        score, dx = cc.score_grad(x, interleaved=interleaved)
        ctx.save_for_backward(dx)
        return score

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        return dx * g.reshape(()), None, None


class _CommittedScoreRaggedFunction(torch.autograd.Function):
    """scores [n_clips] = cc on a padded batch with the gradient kept from the same library call: backward returns dx scaled per clip by
    grad_output[c]."""

    @staticmethod
    def forward(ctx, x, cc, frames, clip_rows, interleaved):
        scores, dx = cc.score_grad_ragged(x, frames, clip_rows, interleaved=interleaved)
        ctx.save_for_backward(dx)
        ctx.rows = [1] * len(frames) if clip_rows is None else [int(r) for r in clip_rows]
        return scores

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        per_row = torch.repeat_interleave(g.reshape(-1).to(torch.float32), torch.tensor(ctx.rows, device=g.device))
        return dx * per_row.reshape(-1, 1, 1), None, None, None, None


def ragged_layout(in_channels, R, Tmax, frames, clip_rows=None):
    """bsrnn_critic_ragged_layout as a dict: the frames behind the four layers at Tmax, the K slabs of the first layer, its frame tiles
    per row and the live ones over all rows, the dx kernel's position tiles likewise, the workspace in floats of a score, of a score
    with its gradient and with the exact chain's planar copies, the bytes of the call's two tables."""
    fr = [int(t) for t in frames]
    rows = [1] * len(fr) if clip_rows is None else [int(r) for r in clip_rows]
    out = (ctypes.c_int64 * 14)()
    _native.check(_lib.bsrnn_critic_ragged_layout(in_channels, R, Tmax, (ctypes.c_int32 * len(fr))(*fr), (ctypes.c_int32 * len(rows))(*rows),
                                                  len(fr), out))
    v = list(out)
    return dict(frames=v[0:4], slabs=v[4], ch_per_slab=v[5], t_tiles=v[6], live_t_tiles=v[7], s_tiles=v[8], live_s_tiles=v[9],
                ws_score_floats=v[10], ws_floats=v[11], ws_exact_floats=v[12], table_bytes=v[13])


def layer1_dx_ragged(cc, dp, Tmax, frames, clip_rows=None, interleaved=False):
    """The first layer's dx alone on a padded batch (bsrnn_critic_layer1_dx_ragged; test and measurement support): dp
    [R, 1024, frames_out(Tmax)], zeros behind each row's own length -> dx [R, in_channels, Tmax], the scale formed per clip."""
    cc._open(grad=True)
    if not isinstance(dp, torch.Tensor) or dp.dim() != 3 or tuple(dp.shape[1:]) != (WIDTHS[0], frames_out(Tmax)):
        raise ValueError("layer1_dx_ragged: expected dp [R, %d, %d], got %s" % (WIDTHS[0], frames_out(Tmax), tuple(getattr(dp, "shape", ()))))
    if dp.device != cc.device:
        raise ValueError("layer1_dx_ragged: dp must be on %s" % (cc.device,))
    dp = _f32c(dp)
    R = dp.shape[0]
    fr, rows = cc._clips("layer1_dx_ragged", frames, clip_rows, R, Tmax)
    with torch.cuda.device(cc.device):
        dx = torch.empty((R, cc.in_channels, Tmax), device=cc.device)
        _native.check(_lib.bsrnn_critic_layer1_dx_ragged(cc._h, _p(dp), R, Tmax, fr, rows, len(fr), int(bool(interleaved)), _p(dx), _s(cc.device)))
    return dx


def layer1_dx(cc, dp, T, interleaved=False):
    """The first layer's dx alone (bsrnn_critic_layer1_dx; test and measurement support): dp [C, 1024, frames_out(T)] -> dx
    [C, in_channels, T] on the path `score_grad` takes, rows in the interleaved order when asked."""
    cc._open(grad=True)
    if not isinstance(dp, torch.Tensor) or dp.dim() != 3 or tuple(dp.shape[1:]) != (WIDTHS[0], frames_out(T)):
        raise ValueError("layer1_dx: expected dp [C, %d, %d], got %s" % (WIDTHS[0], frames_out(T), tuple(getattr(dp, "shape", ()))))
    if dp.device != cc.device:
        raise ValueError("layer1_dx: dp must be on %s" % (cc.device,))
    dp = _f32c(dp)
    C = dp.shape[0]
    with torch.cuda.device(cc.device):
        dx = torch.empty((C, cc.in_channels, T), device=cc.device)
        _native.check(_lib.bsrnn_critic_layer1_dx(cc._h, _p(dp), C, T, int(bool(interleaved)), _p(dx), _s(cc.device)))
    return dx


class CommittedCritic:
    """A frozen Discriminator as an object of the library (bsrnn_critic_*): `Discriminator.commit()` makes one.  It holds a SNAPSHOT -
    its own fp32 copy of every parameter and the first layer as two fp16 pieces, `score_layout(...)["snapshot_bytes"]` and
    `["image_bytes"]`, about 2 x 134 MB at 2050 channels - so the module may train on; `recommit(D)` follows it.  `score` is one library
    call, carries no graph and follows the context's compute mode and range policy like the model entry points.  grad=True
    (`Discriminator.commit(grad=True)`) adds the gradient: a second image of the first layer (`grad_layout(...)["image_bytes"]`),
    `score_grad` and `score_fixed`."""

    def __init__(self, module, grad=False):
        if not isinstance(module, Discriminator):
            raise TypeError("CommittedCritic: expected a Discriminator, got %s" % type(module).__name__)
        dev = next(module.parameters()).device
        if dev.type != "cuda":
            raise ValueError("CommittedCritic: the critic's kernels run on the GPU: move the Discriminator to a cuda device first (there is no CPU fallback)")
        self.in_channels = module.in_channels
        self.device = dev
        self._h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            _native.check(_lib.bsrnn_critic_create(_context(dev), self.in_channels, ctypes.byref(self._h)))
            self.has_grad = bool(grad)
            if grad:
                _native.check(_lib.bsrnn_critic_enable_grad(self._h, _s(dev)))
        self.recommit(module)

    def recommit(self, module):
        """Take a new snapshot of `module` (same in_channels, same device)."""
        if self._h is None:
            raise ValueError("CommittedCritic: closed")
        if not isinstance(module, Discriminator) or module.in_channels != self.in_channels:
            raise ValueError("CommittedCritic.recommit: expected a Discriminator(%d)" % self.in_channels)
        convs = [m for m in module.layers if isinstance(m, nn.Conv1d)]
        lin = module.layers2[0]
        keep = [_f32c(t) for m in convs for t in (m.weight, m.bias)] + [_f32c(lin.weight), _f32c(lin.bias)]
        if any(t.device != self.device for t in keep):
            raise ValueError("CommittedCritic.recommit: the module is not on %s" % (self.device,))
        w = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in keep[0:8:2]])
        b = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in keep[1:8:2]])
        with torch.cuda.device(self.device):
            _native.check(_lib.bsrnn_critic_commit(self._h, w, b, _p(keep[8]), _p(keep[9]), _s(self.device)))     # (synchronous: `keep` may go)
        return self

    def _open(self, grad=False):
        if self._h is None:
            raise ValueError("CommittedCritic: closed")
        if grad and not self.has_grad:
            raise ValueError("CommittedCritic: this object has no gradient: commit(grad=True) makes one that has")

    def _checked(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError("CommittedCritic: expected x [C, %d, T], got %s" % (self.in_channels, tuple(getattr(x, "shape", ()))))
        if x.shape[2] < MIN_FRAMES:
            raise ValueError("CommittedCritic: x has %d frames, the four layers need at least %d (%d samples at hop 1024)" % (
                x.shape[2], MIN_FRAMES, (MIN_FRAMES - 1) * 1024))
        if x.device != self.device:
            raise ValueError("CommittedCritic: x must be on %s, the committed critic's device (there is no CPU fallback)" % (self.device,))
        return _f32c(x)

    def score(self, x, interleaved=False, return_y1=False):
        """x [C, in_channels, T] on the device, T >= 601 -> the score [1] (no graph).  interleaved=True: x is the separator's spectrum
        (re, im, re, im, ...) and is read through the channel map, without the `reference_channel_order` copy.  return_y1: also the
        first layer's output [C, 1024, T1] (test and measurement support)."""
        self._open()
        x = self._checked(x)
        C, _, T = x.shape
        with torch.cuda.device(self.device):
            out = torch.empty((1,), device=self.device)
            y1 = torch.empty((C, WIDTHS[0], frames_out(T)), device=self.device) if return_y1 else None
            _native.check(_lib.bsrnn_critic_score(self._h, _p(x), C, T, int(bool(interleaved)), _p(out), _p(y1), _s(self.device)))
        return (out, y1) if return_y1 else out

    def score_grad(self, x, interleaved=False, gscale=None):
        """x as for `score` -> (score [1], dx [C, in_channels, T]) from ONE library call: the bits `score` gives, and
        gscale * d score / d x in x's own channel order (interleaved=True: the gradient of the separator's spectrum as it lies).
        gscale: None (1) or a one-element float tensor on the device.  Neither carries a graph.  Needs commit(grad=True)."""
        self._open(grad=True)
        x = self._checked(x)
        C, _, T = x.shape
        if gscale is not None:
            if not isinstance(gscale, torch.Tensor) or gscale.numel() != 1 or gscale.device != self.device:
                raise ValueError("CommittedCritic.score_grad: gscale must be a one-element tensor on %s" % (self.device,))
            gscale = _f32c(gscale.detach())
        with torch.cuda.device(self.device):
            out = torch.empty((1,), device=self.device)
            dx = torch.empty_like(x)
            _native.check(_lib.bsrnn_critic_score_grad(self._h, _p(x.detach()), C, T, int(bool(interleaved)), _p(gscale), _p(out), _p(dx),
                                                       _s(self.device)))
        return out, dx

    def score_fixed(self, x, interleaved=False):
        """The score [1] with a graph into x and nowhere else (the critic is frozen): forward makes the one `score_grad` call and keeps
        dx - it is formed while the activations stand in the shared workspace - and backward returns dx * grad_output."""
        self._open(grad=True)
        return _CommittedScoreFunction.apply(x, self, bool(interleaved))

    def _clips(self, who, frames, clip_rows, R, Tmax):
        """(frames, rows per clip) as int32 arrays, or ValueError for what the library refuses by clip."""
        try:
            fr = [int(t) for t in frames]
            rows = [1] * len(fr) if clip_rows is None else [int(r) for r in clip_rows]
        except TypeError:
            raise ValueError("CommittedCritic.%s: frames and clip_rows must be sequences of ints" % who) from None
        if not fr or len(rows) != len(fr):
            raise ValueError("CommittedCritic.%s: %d frame counts and %d row counts, need one of each per clip and at least one clip" % (
                who, len(fr), len(rows)))
        for c, (t, n) in enumerate(zip(fr, rows)):
            if n < 1:
                raise ValueError("CommittedCritic.%s: clip %d has %d rows, need at least 1" % (who, c, n))
            if not MIN_FRAMES <= t <= Tmax:
                raise ValueError("CommittedCritic.%s: clip %d has %d frames, need %d <= frames <= %d (the four layers need %d)" % (
                    who, c, t, MIN_FRAMES, Tmax, MIN_FRAMES))
        if sum(rows) != R:
            raise ValueError("CommittedCritic.%s: the clips own %d rows, the batch has %d" % (who, sum(rows), R))
        return (ctypes.c_int32 * len(fr))(*fr), (ctypes.c_int32 * len(rows))(*rows)

    def _checked_ragged(self, who, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError("CommittedCritic.%s: expected x [R, %d, Tmax], got %s" % (who, self.in_channels, tuple(getattr(x, "shape", ()))))
        if x.device != self.device:
            raise ValueError("CommittedCritic.%s: x must be on %s, the committed critic's device (there is no CPU fallback)" % (who, self.device))
        return _f32c(x)

    def score_ragged(self, x, frames, clip_rows=None, interleaved=False, return_y1=False):
        """One score per clip of a padded batch, in ONE library call (bsrnn_critic_score_ragged): x [R, in_channels, Tmax] on the device;
        clip c owns clip_rows[c] consecutive rows (None: one row per clip) of frames[c] frames each, 601 <= frames[c] <= Tmax; what lies
        behind a row's frames is never read.  -> scores [n_clips] (no graph): for every clip what `score` gives for it alone, up to the
        order of the first layer's sums.  return_y1: also the first layer's output [R, 1024, frames_out(Tmax)], valid below each row's
        own length (test and measurement support)."""
        self._open()
        x = self._checked_ragged("score_ragged", x)
        R, _, Tmax = x.shape
        fr, rows = self._clips("score_ragged", frames, clip_rows, R, Tmax)
        with torch.cuda.device(self.device):
            out = torch.empty((len(fr),), device=self.device)
            y1 = torch.empty((R, WIDTHS[0], frames_out(Tmax)), device=self.device) if return_y1 else None
            _native.check(_lib.bsrnn_critic_score_ragged(self._h, _p(x), R, Tmax, fr, rows, len(fr), int(bool(interleaved)), _p(out), _p(y1),
                                                         _s(self.device)))
        return (out, y1) if return_y1 else out

    def score_grad_ragged(self, x, frames, clip_rows=None, interleaved=False, gscale=None):
        """x, frames, clip_rows as for `score_ragged` -> (scores [n_clips], dx [R, in_channels, Tmax]) from ONE library call: the bits
        `score_ragged` gives, and gscale[c] * d score_c / d x in the rows of clip c, in x's own layout, zeros behind a row's frames.
        gscale: None (1) or a float tensor [n_clips] on the device.  Neither carries a graph.  Needs commit(grad=True)."""
        self._open(grad=True)
        x = self._checked_ragged("score_grad_ragged", x)
        R, _, Tmax = x.shape
        fr, rows = self._clips("score_grad_ragged", frames, clip_rows, R, Tmax)
        if gscale is not None:
            if not isinstance(gscale, torch.Tensor) or gscale.numel() != len(fr) or gscale.device != self.device:
                raise ValueError("CommittedCritic.score_grad_ragged: gscale must be a tensor of %d values on %s" % (len(fr), self.device))
            gscale = _f32c(gscale.detach().reshape(-1))
        with torch.cuda.device(self.device):
            out = torch.empty((len(fr),), device=self.device)
            dx = torch.empty_like(x)
            _native.check(_lib.bsrnn_critic_score_grad_ragged(self._h, _p(x.detach()), R, Tmax, fr, rows, len(fr), int(bool(interleaved)),
                                                              _p(gscale), _p(out), _p(dx), _s(self.device)))
        return out, dx

    def score_fixed_ragged(self, x, frames, clip_rows=None, interleaved=False):
        """The scores [n_clips] with a graph into x and nowhere else: forward makes the one `score_grad_ragged` call and keeps dx,
        backward returns dx scaled per clip by grad_output[c]."""
        self._open(grad=True)
        return _CommittedScoreRaggedFunction.apply(x, self, [int(t) for t in frames], None if clip_rows is None else [int(r) for r in clip_rows],
                                                   bool(interleaved))

    def close(self):
        """Free the snapshot and the image (idempotent)."""
        if getattr(self, "_h", None) is not None:
            _lib.bsrnn_critic_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CriticConvFunction(torch.autograd.Function):
    """y = act(conv1d(x, w, b, stride=3)) with the library's forward and backward: apply(x [C, I, T], w [O, I, 16], b [O], leaky)
    -> [C, O, T_out]; leaky selects LeakyReLU(0.01).  dx is only formed when x wants a gradient."""

    @staticmethod
    def forward(ctx, x, w, b, leaky):
        if not x.is_cuda:
            raise ValueError("the critic's kernels run on the GPU: x must be a cuda tensor")
        x, w, b = _f32c(x), _f32c(w), _f32c(b)
        C, I, T = x.shape
        O = w.shape[0]
        if tuple(w.shape) != (O, I, KERNEL) or tuple(b.shape) != (O,):
            raise ValueError("critic layer: weight %s / bias %s do not match x [C, %d, T]" % (tuple(w.shape), tuple(b.shape), I))
        dev = x.device
        with torch.cuda.device(dev):
            y = torch.empty((C, O, frames_out(T)), device=dev)
            _native.check(_lib.bsrnn_critic_conv_forward(_context(dev), _p(x), _p(w), _p(b), _p(y), C, I, T, O, int(bool(leaky)), _s(dev)))
        ctx.save_for_backward(x, w, y)
        ctx.leaky = bool(leaky)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        C, I, T = x.shape
        O = w.shape[0]
        dy = _f32c(dy)
        dev = x.device
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dw, db = torch.empty_like(w), torch.empty((O,), device=dev)
            _native.check(_lib.bsrnn_critic_conv_backward(_context(dev), _p(x), _p(w), _p(y), _p(dy), _p(dx), _p(dw), _p(db), C, I, T, O,
                                                          int(ctx.leaky), _s(dev)))
        return dx, dw, db, None


class Discriminator(nn.Module):
    """bsrnn.py:512-536.  `state_dict()` is the reference's, key for key and shape for shape (`layers.{0,2,4,6}.{weight,bias}`,
    `layers2.0.{weight,bias}`), so `discriminator.pth` interchanges.

    in_channels: the reference hard-codes 4098 = 2 * 2049, the channels of the 4096-point transform of train-discriminator.py:64;
    `critic_spectrum` forms that input, and `train-discriminator.py --n_fft 4096` trains this default critic on it.  The default is
    stale in the reference's other caller: m_dataset.train_infer feeds the critic `cat(real, imag)` of the model's 2048-point output,
    2050 channels, so its own call raises with the default critic.  `Discriminator(2050)` is the size `metrics.train_infer`,
    `train.train_loss` and `train-discriminator.py` at its default `--n_fft 2048` use."""

    def __init__(self, in_channels=4098):
        super().__init__()
        self.in_channels = int(in_channels)
        dims = (self.in_channels,) + WIDTHS
        mods = []
        for l in range(len(WIDTHS)):
            mods.append(nn.Conv1d(dims[l], dims[l + 1], KERNEL, stride=STRIDE))
            if l + 1 < len(WIDTHS):
                mods.append(nn.LeakyReLU())
        self.layers = nn.Sequential(*mods)
        self.layers2 = nn.Sequential(nn.Linear(WIDTHS[-1], 1), nn.Sigmoid())

    def forward(self, x):
        """x [C, in_channels, T] on the device, T >= 601 -> the score [1]."""
        return self._score(x, fixed=False)

    def score_fixed(self, x):
        """forward with the critic's parameters held fixed: the gradient flows through the critic into x and nowhere else (the
        adversarial term of train.train_loss)."""
        return self._score(x, fixed=True)

    def commit(self, grad=False):
        """The module as it stands, frozen into a CommittedCritic (a snapshot: later changes of the parameters do not reach it).
        grad=True: the object also serves d score / d x (`score_grad`, `score_fixed`), at the price of a second first-layer image."""
        return CommittedCritic(self, grad=grad)

    def _score(self, x, fixed):
        if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.shape[1] != self.in_channels:
            raise ValueError("Discriminator: expected x [C, %d, T], got %s" % (self.in_channels, tuple(getattr(x, "shape", ()))))
        if x.shape[2] < MIN_FRAMES:
            raise ValueError("Discriminator: x has %d frames, the four layers need at least %d (%d samples at hop 1024)" % (
                x.shape[2], MIN_FRAMES, (MIN_FRAMES - 1) * 1024))
        if not x.is_cuda:
            raise ValueError("Discriminator: the critic's kernels run on the GPU: x must be a cuda tensor (there is no CPU fallback)")
        par = (lambda p: p.detach()) if fixed else (lambda p: p)       # noqa: E731
        h = x
        convs = [m for m in self.layers if isinstance(m, nn.Conv1d)]
        for l, m in enumerate(convs):
            h = CriticConvFunction.apply(h, par(m.weight), par(m.bias), l + 1 < len(convs))
        h = h.mean(dim=2).mean(dim=0)                                   # bsrnn.py:533-534
        lin = self.layers2[0]
        return torch.sigmoid(LinearFunction.apply(h.reshape(1, -1), par(lin.weight), par(lin.bias), False).reshape(1))
