"""Host-side mirror of the reference's `bsrnn.py` operator interface, running on libbsrnn_hip.

Same surface as the reference model class (bsrnn.py:328-510):
    BSRNN()                                   no constructor arguments (band table optional here)
    .to(device) / .eval() / .state_dict() / .load_state_dict(sd)   -- identical key names and
                                              shapes (288 tensors)
    .forward(x [C,2050,T]) -> [C,2050,T]      bsrnn.py:385
    .forward_recurrent(x [C,2050], state [4,2,C*K,64]) -> (y, new_state)   bsrnn.py:445
    generate_bandsplits(), band_features, merge_channels module globals    bsrnn.py:247, :60-61
plus the fused device-side sandwich of the callers (`separate`, `stft`, `istft`) and the chunked
streaming form.  The torch modules below are *parameter containers only* (they give the
state_dict its names, shapes and default initialisation); their own forward() is never
called -- all arithmetic happens in hand-written HIP kernels behind the C ABI, and without
the built library this module cannot be imported (no CPU fallback).
"""
import ctypes
import math

import numpy as np
import torch
from torch import nn

from . import _native
from . import spec as _spec
from .spec import generate_bandsplits  # noqa: F401  (re-export, bsrnn.py:247)
from .discriminator import Discriminator  # noqa: F401  (re-export, bsrnn.py:512: `from bsrnn import Discriminator` of train.py:12)

band_features = _spec.BAND_FEATURES      # bsrnn.py:60
merge_channels = _spec.MERGE_CHANNELS    # bsrnn.py:61
_lib = _native.lib
_check = _native.check


class TrainableConstantModule(nn.Module):
    """Parameter container for the zero-width band's learned constant (bsrnn.py:12-24)."""

    def __init__(self, shape):
        super().__init__()
        self.trainable_constant = nn.Parameter(torch.zeros(shape, dtype=torch.float32))


def _mlp(dims, act_after_last):
    """Sequential whose even slots hold Linear(dims[i] -> dims[i+1]) so that the parameter
    names come out as `<i*2>.weight/.bias` like the reference's Sequentials."""
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2 or act_after_last:
            mods.append(nn.LeakyReLU())
    return nn.Sequential(*mods)


class _RNNBlockParams(nn.Module):
    """fc_in / rnn / fc of NormRNNResidual (bsrnn.py:63-76), as containers."""

    def __init__(self, bidirectional):
        super().__init__()
        H = band_features
        self.fc_in = nn.Linear(H, H)
        self.rnn = nn.LSTM(H, H, batch_first=True, num_layers=2, bidirectional=bidirectional)
        self.fc = nn.Linear(2 * H if bidirectional else H, H)


class _Holder(nn.Module):
    def __init__(self, bidirectional):
        super().__init__()
        self.m = _RNNBlockParams(bidirectional)


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class BSRNN(nn.Module):
    def __init__(self, band_widths=None):
        super().__init__()
        v = list(band_widths) if band_widths is not None else generate_bandsplits()[0]
        self.band_widths = v
        H, MH = band_features, _spec.MASK_HIDDEN
        self.bandFCs_pre = nn.ModuleList(
            [_mlp([2 * w, 2 * w, 2 * w], True) if w > 0 else nn.Sequential(TrainableConstantModule([0])) for w in v])
        self.bandFCs = nn.ModuleList(
            [_mlp([2 * w, max(2 * w, H), H, H], False) if w > 0 else nn.Sequential(TrainableConstantModule([H])) for w in v])
        self.lstms = nn.Sequential(_Holder(True), _Holder(False), _Holder(True), _Holder(False))
        self.bandFCs_back = nn.ModuleList(
            [_mlp([H, MH, max(2 * w, MH), 2 * w], True) if w > 0 else nn.Sequential(TrainableConstantModule(0)) for w in v])
        self.bandFCs_back_post = nn.ModuleList(
            [_mlp([2 * w, 2 * w, 2 * w], False) if w > 0 else nn.Sequential(TrainableConstantModule([0])) for w in v])
        self._ctx = None
        self._ctx_device = None
        self._pushed_fingerprint = None
        self._plist = None                  # cached parameter tensors (the module tree is fixed after construction)
        self._pident = ()                   # their (id, data_ptr) pairs when the list was built
        self._epoch = 0                     # bumped by everything that may rebind parameter storage (_apply, load_state_dict)
        self._range_policy = _native.RANGE_EXACT

    # ------------------------------------------------------------------ native context / weights
    def __del__(self):
        try:
            if self._ctx is not None:
                _lib.bsrnn_destroy(self._ctx)
        except Exception:
            pass

    def _fingerprint(self):
        """Cheap identity of the current weights: every in-place edit of a parameter bumps its tensor's `_version`; `.to()` /
        `.cuda()` / `.float()` (all through `_apply`) and `load_state_dict` bump `_epoch`; rebinding a parameter's storage
        (`p.data = t`, `module.weight = Parameter(...)`, `swap_tensors`) changes the (id, data_ptr) pairs taken when the
        parameter list is (re)built.  One attribute read per parameter per check."""
        if self._plist is None:
            self._plist = list(self.parameters())
            self._pident = tuple((id(p), p.data_ptr()) for p in self._plist)
        return (self._epoch, self._pident) + tuple(p._version for p in self._plist)

    def _weights_touched(self, k, n=8):
        """Slice k of n of the cached parameter list: has any of them been edited in place or had its storage rebound since
        the last upload?  (The streaming wrapper calls this every step with a rotating k: an optimizer step or any other
        edit of ALL parameters is seen at the very next chunk, an edit of ONE tensor within n chunks, for ~3 us per step.)"""
        fp = self._pushed_fingerprint
        if fp is None or self._plist is None:
            return True
        pl, ident, vers = self._plist, fp[1], fp[2:]
        for i in range(k % n, len(pl), n):
            p = pl[i]
            if p._version != vers[i] or p.data_ptr() != ident[i][1]:
                return True
        return False

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._plist = None
        self._epoch += 1
        self._pushed_fingerprint = None     # (also tells a running StreamingSeparator to look at the weights at its next step)
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._plist = None
        self._epoch += 1
        self._pushed_fingerprint = None
        return out

    def set_range_policy(self, policy):
        """'exact' (default): every call waits for its kernels and, if an activation left the fp16x2 range (|a| > 65504),
        is run again on the exact-fp32 kernels before it returns - results always match the reference's forward.
        'deferred': calls return without waiting (benchmark loops, launch pipelines); a violation surfaces as a NativeError
        at the next call on this model (include/bsrnn_hip.h, bsrnn_set_range_policy)."""
        self._range_policy = {"exact": _native.RANGE_EXACT, "deferred": _native.RANGE_DEFERRED}[policy]
        if self._ctx is not None:
            _check(_lib.bsrnn_set_range_policy(self._ctx, self._range_policy))

    def _context(self, device):
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        if self._ctx is None or self._ctx_device != dev_index:
            if self._ctx is not None:
                _lib.bsrnn_destroy(self._ctx)
                self._ctx = None
            widths = (ctypes.c_int32 * len(self.band_widths))(*self.band_widths)
            ctx = ctypes.c_void_p()
            _check(_lib.bsrnn_create(dev_index, widths, len(self.band_widths), ctypes.byref(ctx)))
            self._ctx, self._ctx_device, self._pushed_fingerprint = ctx, dev_index, None
            _check(_lib.bsrnn_set_range_policy(ctx, self._range_policy))
        fp = self._fingerprint()
        if fp != self._pushed_fingerprint:
            for key, val in self.state_dict().items():
                a = np.ascontiguousarray(val.detach().to("cpu", torch.float32).numpy())
                _check(_lib.bsrnn_set_param(self._ctx, key.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size))
            _check(_lib.bsrnn_commit_params(self._ctx))
            self._pushed_fingerprint = fp
        return self._ctx

    def mlp_flow(self, device=None):
        """'fused' (one launch per MLP chain, the default) or 'layers' (one grouped launch per Linear layer) on `device`."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return "fused" if _lib.bsrnn_mlp_fused(self._context(dev)) == 1 else "layers"

    def chain_geometry(self, chain, band, device=None):
        """(rows per workgroup, MFMA shape, RT, NW, rag layer bits, pad zeroing) of band `band`'s fused chain `chain` (0 split,
        1 mask); all 0 for a zero-width band, all -1 under the per-layer flow (include/bsrnn_hip.h, bsrnn_chain_geometry)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        out = (ctypes.c_int32 * 6)()
        _check(_lib.bsrnn_chain_geometry(self._context(dev), chain, band, out))
        return tuple(out)

    def overlap_state(self, device=None):
        """How this model's context runs the dual path of large calls: 1 overlapped (default), 0 launch after launch (BSRNN_OVERLAP=0),
        2 switched off after a consumer's wait expired (include/bsrnn_hip.h, bsrnn_overlap_state)."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return _lib.bsrnn_overlap_state(self._context(dev))

    def sync(self, device=None):
        """Wait for this model's work on the current stream of `device`; raises if a call made under the 'deferred' range
        policy left the fp16x2 range (bsrnn_sync)."""
        dev = torch.device("cuda", self._ctx_device if self._ctx_device is not None else torch.cuda.current_device()) if device is None else torch.device(device)
        if self._ctx is not None:
            with torch.cuda.device(dev):
                _check(_lib.bsrnn_sync(self._ctx, _stream_ptr(dev)))

    def refresh_weights(self):
        """Force re-upload (only needed after edits that bypass tensor versioning, e.g. `p.data = other`)."""
        self._pushed_fingerprint = None
        self._plist = None

    @staticmethod
    def _device_for(x):
        if x.is_cuda:
            return x.device
        if not torch.cuda.is_available():
            raise _native.NativeError("BSRNN needs a HIP device: no GPU visible and there is no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device())

    @staticmethod
    def _prep(x, dev):
        return x.detach().to(device=dev, dtype=torch.float32).contiguous()

    # ------------------------------------------------------------------ reference interface
    def forward(self, x):
        """bsrnn.py:385: x [C, 2050, T] (re/im interleaved STFT) -> x * mask, same shape."""
        return self._forward(x, want_mask=False)[0]

    def forward_with_mask(self, x):
        """forward plus the mask itself (bsrnn.py:425-432), for parity checks."""
        return self._forward(x, want_mask=True)

    def _forward(self, x, want_mask):
        if x.dim() != 3 or x.shape[1] != _spec.N_BINS * 2:
            raise ValueError("expected x [C, 2050, T], got %s" % (tuple(x.shape),))
        dev = self._device_for(x)
        xd = self._prep(x, dev)
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            y = torch.empty_like(xd)
            mask = torch.empty_like(xd) if want_mask else None
            _check(_lib.bsrnn_forward(ctx, _ptr(xd), _ptr(y), _ptr(mask) if want_mask else None,
                                      xd.shape[0], xd.shape[2], _stream_ptr(dev)))
        if not x.is_cuda:
            y = y.cpu()
            mask = mask.cpu() if want_mask else None
        return y, mask

    def forward_recurrent(self, x, state):
        """bsrnn.py:445: one frame.  x [C, 2050], state [4, 2, C*K, 64] -> (y, new_state)."""
        if x.dim() != 2 or x.shape[1] != _spec.N_BINS * 2:
            raise ValueError("expected x [C, 2050], got %s" % (tuple(x.shape),))
        y, ns = self.forward_chunk(x.unsqueeze(2), state)
        return y.squeeze(2), ns

    def forward_chunk(self, x, state):
        """L consecutive frames with causal state carry: x [C, 2050, L]."""
        C, _, L = x.shape
        K = len(self.band_widths)
        if tuple(state.shape) != (4, 2, C * K, band_features):
            raise ValueError("expected state [4, 2, %d, 64], got %s" % (C * K, tuple(state.shape)))
        dev = self._device_for(x)
        xd, sd = self._prep(x, dev), self._prep(state, dev)
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            y, ns = torch.empty_like(xd), torch.empty_like(sd)
            _check(_lib.bsrnn_forward_chunk(ctx, _ptr(xd), _ptr(sd), _ptr(y), _ptr(ns), C, L, _stream_ptr(dev)))
        if not x.is_cuda:
            y, ns = y.cpu(), ns.cpu()
        return y, ns

    def dual_path(self, z, state=None):
        """self.lstms(z) (bsrnn.py:417): z [C, T, K, 64] -> (z_out, new_state)."""
        C, T, K, Hh = z.shape
        if K != len(self.band_widths) or Hh != band_features:
            raise ValueError("expected z [C, T, %d, 64]" % len(self.band_widths))
        dev = self._device_for(z)
        zd = self._prep(z, dev)
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            out = torch.empty_like(zd)
            sd = self._prep(state, dev) if state is not None else torch.zeros((4, 2, C * K, Hh), device=dev)
            ns = torch.empty_like(sd)
            _check(_lib.bsrnn_dual_path(ctx, _ptr(zd), _ptr(out), _ptr(sd), _ptr(ns), C, T, _stream_ptr(dev)))
        if not z.is_cuda:
            out, ns = out.cpu(), ns.cpu()
        return out, ns

    # ------------------------------------------------------------------ the callers' sandwich, on device
    def stft(self, waveform):
        """infer.py:29-33: [R, n] -> [R, 2050, 1 + n//1024]."""
        dev = self._device_for(waveform)
        w = self._prep(waveform, dev)
        R, n = w.shape
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            x = torch.empty((R, 2 * _spec.N_BINS, 1 + n // _spec.HOP), device=dev, dtype=torch.float32)
            _check(_lib.bsrnn_stft(ctx, _ptr(w), _ptr(x), R, n, _stream_ptr(dev)))
        return x if waveform.is_cuda else x.cpu()

    def istft(self, y):
        """infer.py:35-37: [R, 2050, T] -> [R, (T-1)*1024]."""
        dev = self._device_for(y)
        yd = self._prep(y, dev)
        R, _, T = yd.shape
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            out = torch.empty((R, (T - 1) * _spec.HOP), device=dev, dtype=torch.float32)
            _check(_lib.bsrnn_istft(ctx, _ptr(yd), _ptr(out), R, T, _stream_ptr(dev)))
        return out if y.is_cuda else out.cpu()

    def separate(self, waveform, out=None):
        """STFT -> forward -> iSTFT fused on the device: [R, n] -> [R, (n//1024)*1024].  `out`, if given, must be a contiguous
        float32 tensor of exactly that shape on the call's device (the kernels write it whole) and must not overlap the waveform."""
        dev = self._device_for(waveform)
        w = self._prep(waveform, dev)
        R, n = w.shape
        shape = (R, (n // _spec.HOP) * _spec.HOP)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev
                                or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError("separate: out must be a contiguous float32 tensor %s on %s, got %s" % (
                shape, dev, "%s %s on %s" % (tuple(out.shape), out.dtype, out.device) if isinstance(out, torch.Tensor) else type(out).__name__))
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            if out is None:
                out = torch.empty(shape, device=dev, dtype=torch.float32)
            _check(_lib.bsrnn_separate(ctx, _ptr(w), _ptr(out), R, n, _stream_ptr(dev)))
        return out if waveform.is_cuda else out.cpu()

    def separate_long(self, waveform, segment_frames=256, out=None):
        """`separate` for a clip of any length in bounded memory: [R, n] -> [R, (n//1024)*1024], the frames cut into segments of
        `segment_frames` (LSTM state and overlap-add tail carried from segment to segment; include/bsrnn_hip.h, bsrnn_separate_long).
        The library's workspace is that of one segment.  A CUDA tensor is separated on its device; a CPU tensor stays on the host -
        the library streams it through pinned windows, so the device holds O(R * segment_frames) of it, never the clip - and the
        result is a CPU tensor.  `out` as in `separate`: contiguous float32 of exactly the result's shape on the waveform's device,
        not overlapping it.  segment_frames >= the clip's frames is `separate` itself (bit-identical).  The default of 256 frames is
        the chunk length of the chunked benchmark configuration, not a measured optimum."""
        if not isinstance(waveform, torch.Tensor) or waveform.dim() != 2:
            raise ValueError("separate_long: expected waveform [R, n], got %s" % (
                tuple(waveform.shape) if isinstance(waveform, torch.Tensor) else type(waveform).__name__,))
        dev = self._device_for(waveform)
        on_host = not waveform.is_cuda
        w = waveform.detach().to(dtype=torch.float32).contiguous() if on_host else self._prep(waveform, dev)
        R, n = w.shape
        shape = (R, (n // _spec.HOP) * _spec.HOP)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != w.device
                                or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError("separate_long: out must be a contiguous float32 tensor %s on %s, got %s" % (
                shape, w.device, "%s %s on %s" % (tuple(out.shape), out.dtype, out.device) if isinstance(out, torch.Tensor) else type(out).__name__))
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            if out is None:
                out = torch.empty(shape, device=w.device, dtype=torch.float32)
            if on_host:
                _check(_lib.bsrnn_separate_long_host(ctx, _ptr(w), _ptr(out), R, n, int(segment_frames)))
            else:
                _check(_lib.bsrnn_separate_long(ctx, _ptr(w), _ptr(out), R, n, int(segment_frames), _stream_ptr(dev)))
        return out

    def separate_ragged(self, waveform, lengths, out=None):
        """`separate` for clips of different lengths in one call: waveform [R, n_max], row r holding lengths[r] samples (1024 < lengths[r]
        <= n_max; what lies behind them in the row is never read) -> [R, (Tmax - 1) * 1024], Tmax = 1 + max(lengths) // 1024.  Row r holds
        the (lengths[r] // 1024) * 1024 samples `separate` gives for that clip alone (to rounding; bit-identical when all lengths are n_max),
        then zeros.  The model runs on all R * Tmax frame rows: padding is paid for (include/bsrnn_hip.h, bsrnn_separate_ragged;
        `separate_many` batches clips of similar length).  `out` as in `separate`: contiguous float32 of exactly the result's shape on the
        call's device, not overlapping the waveform."""
        if not isinstance(waveform, torch.Tensor) or waveform.dim() != 2:
            raise ValueError("separate_ragged: expected waveform [R, n_max], got %s" % (
                tuple(waveform.shape) if isinstance(waveform, torch.Tensor) else type(waveform).__name__,))
        R, n_max = waveform.shape
        try:
            lens = [int(x) for x in lengths]
        except TypeError:
            raise ValueError("separate_ragged: lengths must be a sequence of %d ints, got %s" % (R, type(lengths).__name__)) from None
        if len(lens) != R or R < 1:
            raise ValueError("separate_ragged: %d lengths for %d rows" % (len(lens), R))
        for r, n in enumerate(lens):
            if not _spec.HOP < n <= n_max:
                raise ValueError("separate_ragged: row %d has %d samples, need 1024 < length <= %d" % (r, n, n_max))
        shape = (R, (max(lens) // _spec.HOP) * _spec.HOP)
        if out is not None and not isinstance(out, torch.Tensor):
            raise ValueError("separate_ragged: out must be a tensor, got %s" % type(out).__name__)
        dev = self._device_for(waveform)
        if out is not None and (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError("separate_ragged: out must be a contiguous float32 tensor %s on %s, got %s %s on %s" % (
                shape, dev, tuple(out.shape), out.dtype, out.device))
        w = self._prep(waveform, dev)
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            if out is None:
                out = torch.empty(shape, device=dev, dtype=torch.float32)
            _check(_lib.bsrnn_separate_ragged(ctx, _ptr(w), n_max, (ctypes.c_int64 * R)(*lens), _ptr(out), R, _stream_ptr(dev)))
        return out if waveform.is_cuda else out.cpu()

    def separate_many(self, clips, max_rows=64, max_padding=0.25):
        """`separate` for a list of clips of different lengths, batched: clips are 1-D [n] or 2-D [ch, n] tensors (n > 1024) on the GPU
        or the CPU.  `spec.ragged_buckets` groups them (longest first; at most `max_rows` rows and a padding share of at most `max_padding`
        per bucket), each bucket is packed into one [rows, n_max] buffer and runs as ONE `separate_ragged` call.  Returns the results in
        input order, each [ch, (n // 1024) * 1024] - 1-D for a 1-D clip - on its clip's own device, equal to `separate` of that clip alone
        to rounding.  max_rows = 64 is the benchmark's batch; max_padding = 0.25 is a default, not a measured optimum."""
        clips = list(clips)
        for i, c in enumerate(clips):
            if not isinstance(c, torch.Tensor) or c.dim() not in (1, 2) or c.shape[-1] <= _spec.HOP or c.shape[0] < 1:
                raise ValueError("separate_many: clip %d must be a tensor [n] or [ch, n] with n > 1024, got %s" % (
                    i, tuple(c.shape) if isinstance(c, torch.Tensor) else type(c).__name__))
        buckets = _spec.ragged_buckets([_spec.n_frames(c.shape[-1]) for c in clips], [1 if c.dim() == 1 else c.shape[0] for c in clips],
                                       max_rows, max_padding)
        if not clips:
            return []
        dev = next((c.device for c in clips if c.is_cuda), None) or self._device_for(clips[0])
        results = [None] * len(clips)
        for bucket in buckets:
            rows = [1 if clips[i].dim() == 1 else clips[i].shape[0] for i in bucket]
            lens = [clips[i].shape[-1] for i in bucket]
            buf = torch.empty((sum(rows), max(lens)), device=dev, dtype=torch.float32)      # (behind a row's end nothing is read)
            r0 = 0
            for i, ch, n in zip(bucket, rows, lens):
                buf[r0:r0 + ch, :n] = clips[i].detach().reshape(ch, n).to(device=dev, dtype=torch.float32)
                r0 += ch
            out = self.separate_ragged(buf, [n for ch, n in zip(rows, lens) for _ in range(ch)])
            r0 = 0
            for i, ch, n in zip(bucket, rows, lens):
                y = out[r0:r0 + ch, :(n // _spec.HOP) * _spec.HOP]
                y = (y[0] if clips[i].dim() == 1 else y).to(clips[i].device, copy=True)
                results[i] = y.contiguous()
                r0 += ch
        return results

    def separate_long_ragged(self, waveform, lengths, segment_frames=256, out=None):
        """`separate_ragged` in segments, for clips that are long AND unequal: waveform [R, n_max], row r holding lengths[r] samples ->
        [R, (Tmax - 1) * 1024] exactly as `separate_ragged` lays it out (each row its clip's samples, then zeros), from a workspace of
        R * segment_frames frame rows.  A row that has ended is absent from later segments, so put the rows LONGEST FIRST: then the model
        runs on about the real frames, rounded up to a segment per row (`spec.long_plan` gives the count); any order gives the same
        result to rounding, a row that ends in front of a longer one is carried as zero frames.  Checks and `out` as `separate_ragged`;
        segment_frames >= Tmax is `separate_ragged` itself, equal lengths are `separate_long` (both bit-identical).  A CPU waveform is
        moved to the device whole (there is no host-buffer variant), the result comes back as a CPU tensor.  The default of 256 frames
        is inherited from `separate_long`, not a measured optimum (include/bsrnn_hip.h, bsrnn_separate_long_ragged)."""
        if not isinstance(waveform, torch.Tensor) or waveform.dim() != 2:
            raise ValueError("separate_long_ragged: expected waveform [R, n_max], got %s" % (
                tuple(waveform.shape) if isinstance(waveform, torch.Tensor) else type(waveform).__name__,))
        R, n_max = waveform.shape
        try:
            lens = [int(x) for x in lengths]
        except TypeError:
            raise ValueError("separate_long_ragged: lengths must be a sequence of %d ints, got %s" % (R, type(lengths).__name__)) from None
        if len(lens) != R or R < 1:
            raise ValueError("separate_long_ragged: %d lengths for %d rows" % (len(lens), R))
        for r, n in enumerate(lens):
            if not _spec.HOP < n <= n_max:
                raise ValueError("separate_long_ragged: row %d has %d samples, need 1024 < length <= %d" % (r, n, n_max))
        try:
            seg = int(segment_frames)
        except (TypeError, ValueError):
            raise ValueError("separate_long_ragged: segment_frames must be an int, got %r" % (segment_frames,)) from None
        if seg < 1:
            raise ValueError("separate_long_ragged: segment_frames = %d (at least one frame per segment)" % seg)
        shape = (R, (max(lens) // _spec.HOP) * _spec.HOP)
        if out is not None and not isinstance(out, torch.Tensor):
            raise ValueError("separate_long_ragged: out must be a tensor, got %s" % type(out).__name__)
        dev = self._device_for(waveform)
        if out is not None and (out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError("separate_long_ragged: out must be a contiguous float32 tensor %s on %s, got %s %s on %s" % (
                shape, dev, tuple(out.shape), out.dtype, out.device))
        w = self._prep(waveform, dev)
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            if out is None:
                out = torch.empty(shape, device=dev, dtype=torch.float32)
            _check(_lib.bsrnn_separate_long_ragged(ctx, _ptr(w), n_max, (ctypes.c_int64 * R)(*lens), _ptr(out), R, seg, _stream_ptr(dev)))
        return out if waveform.is_cuda else out.cpu()

    def separate_many_long(self, clips, segment_frames=256, max_rows=64):
        """`separate_many` for clips that are long and of very different lengths: clips are 1-D [n] or 2-D [ch, n] tensors (n > 1024) on
        the GPU or the CPU.  `spec.long_buckets` sorts them longest first and fills buckets of at most `max_rows` rows - no padding cap,
        the segments bound the padding -, each bucket is packed into one [rows, n_max] buffer, rows longest first, and runs as ONE
        `separate_long_ragged` call.  Returns the results in input order, each [ch, (n // 1024) * 1024] - 1-D for a 1-D clip - on its
        clip's own device, equal to `separate` of that clip alone to rounding."""
        clips = list(clips)
        for i, c in enumerate(clips):
            if not isinstance(c, torch.Tensor) or c.dim() not in (1, 2) or c.shape[-1] <= _spec.HOP or c.shape[0] < 1:
                raise ValueError("separate_many_long: clip %d must be a tensor [n] or [ch, n] with n > 1024, got %s" % (
                    i, tuple(c.shape) if isinstance(c, torch.Tensor) else type(c).__name__))
        try:
            seg = int(segment_frames)
        except (TypeError, ValueError):
            raise ValueError("separate_many_long: segment_frames must be an int, got %r" % (segment_frames,)) from None
        if seg < 1:
            raise ValueError("separate_many_long: segment_frames = %d (at least one frame per segment)" % seg)
        buckets = _spec.long_buckets([_spec.n_frames(c.shape[-1]) for c in clips], [1 if c.dim() == 1 else c.shape[0] for c in clips], max_rows)
        if not clips:
            return []
        dev = next((c.device for c in clips if c.is_cuda), None) or self._device_for(clips[0])
        results = [None] * len(clips)
        for bucket in buckets:
            rows = [1 if clips[i].dim() == 1 else clips[i].shape[0] for i in bucket]
            lens = [clips[i].shape[-1] for i in bucket]
            buf = torch.empty((sum(rows), max(lens)), device=dev, dtype=torch.float32)      # (behind a row's end nothing is read)
            r0 = 0
            for i, ch, n in zip(bucket, rows, lens):
                buf[r0:r0 + ch, :n] = clips[i].detach().reshape(ch, n).to(device=dev, dtype=torch.float32)
                r0 += ch
            out = self.separate_long_ragged(buf, [n for ch, n in zip(rows, lens) for _ in range(ch)], seg)
            r0 = 0
            for i, ch, n in zip(bucket, rows, lens):
                y = out[r0:r0 + ch, :(n // _spec.HOP) * _spec.HOP]
                y = (y[0] if clips[i].dim() == 1 else y).to(clips[i].device, copy=True)
                results[i] = y.contiguous()
                r0 += ch
        return results

    # ------------------------------------------------------------------ sample-rate conversion on the device
    @staticmethod
    def _rows_view(t):
        """(tensor, row stride) of a 2-D float32 cuda tensor for a call that takes rows `stride` floats apart.  The tensor's own stride(0)
        is passed on only where it describes such rows: samples contiguous and rows at least a row's length apart (buf[:, a:b], buf[::2]).
        Every other view is copied: strided samples, and rows that overlap or coincide (mono.expand(2, -1) has stride(0) = 0; unfold and
        as_strided give 0 < stride(0) < n) - the library refuses a stride below the row length."""
        R, n = t.shape
        if (n > 1 and t.stride(1) != 1) or (R > 1 and t.stride(0) < n):
            t = t.contiguous()
        return t, (t.stride(0) if R > 1 else n)

    def resample(self, wave, rate_in, rate_out, out=None):
        """wave [R, n] float32 on a HIP device -> [R, n_out] at rate_out, n_out = ceil(n * up / down): exactly
        scipy.signal.resample_poly(wave, up, down, axis=1) evaluated in fp32 on the device (include/bsrnn_hip.h, bsrnn_resample).  Rows may
        be a view into a wider buffer (wave = buf[:, a:b]): the row stride is passed on and nothing behind a row's n samples is read.  Any
        other view (strided samples, expanded or overlapping rows such as mono.expand(2, -1)) is copied first.  `out`, if given, is a
        float32 tensor [R, n_out] on the same device with contiguous rows at least n_out apart (it may be a view into a wider buffer too);
        it must not overlap the span of the input, first sample of the first row to last sample of the last."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[1] < 1 or wave.shape[0] < 1:
            raise ValueError("resample: expected wave [R, n] with n >= 1, got %s" % (
                tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__,))
        if wave.dtype != torch.float32:
            raise ValueError("resample: expected a float32 tensor, got %s" % wave.dtype)
        R, n = wave.shape
        n_out = resample_len(n, rate_in, rate_out)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != wave.device
                                or tuple(out.shape) != (R, n_out) or (out.stride(1) != 1 and n_out > 1)
                                or (R > 1 and out.stride(0) < n_out)):
            raise ValueError("resample: out must be a float32 tensor %s with contiguous rows that do not overlap on %s, got %s" % (
                (R, n_out), wave.device, "%s %s with strides %s on %s" % (tuple(out.shape), out.dtype, tuple(out.stride()), out.device)
                if isinstance(out, torch.Tensor) else type(out).__name__))
        if not wave.is_cuda:
            raise _native.NativeError("resample: the waveform must be on a HIP device (audio.resample is the host utility)")
        dev = wave.device
        w, w_stride = self._rows_view(wave.detach())
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            if out is None:
                out = torch.empty((R, n_out), device=dev, dtype=torch.float32)
            o_stride = out.stride(0) if R > 1 else n_out
            _check(_lib.bsrnn_resample(ctx, _ptr(w), w_stride, _ptr(out), o_stride, R, n, int(rate_in), int(rate_out), _stream_ptr(dev)))
        return out

    def separate_at_rate(self, wave, sample_rate, model_rate=44100, segment_frames=None):
        """`separate` for audio at another rate than the model's: wave [R, n] float32 on a HIP device at sample_rate -> resample to
        model_rate, `separate` (`separate_long` with segment_frames, if given), resample back - the three public calls chained, all on
        the device - cut to at most n samples (the model returns whole hops, so the result is usually a little shorter than the
        input).  sample_rate == model_rate IS `separate`."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2:
            raise ValueError("separate_at_rate: expected wave [R, n], got %s" % (
                tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__,))
        if int(sample_rate) < 1 or int(model_rate) < 1:
            raise ValueError("separate_at_rate: rates must be at least 1, got %s and %s" % (sample_rate, model_rate))
        if segment_frames is not None and int(segment_frames) < 1:
            raise ValueError("separate_at_rate: segment_frames must be at least 1, got %s" % (segment_frames,))

        def run(w):
            return self.separate(w) if segment_frames is None else self.separate_long(w, int(segment_frames))
        if int(sample_rate) == int(model_rate):
            return run(wave)
        y = self.resample(run(self.resample(wave, sample_rate, model_rate)), model_rate, sample_rate)
        return y[:, :min(wave.shape[1], y.shape[1])]

    def workspace_rows(self, device=None):
        """Frame rows the native context's workspace holds right now (grow-only; 0 before the first call): what `separate` raises to
        R * T and `separate_long` keeps at R * segment_frames (bsrnn_workspace_rows).  `device`: only the context on that device counts."""
        if self._ctx is None:
            return 0
        if device is not None:
            d = torch.device(device)
            if (d.index if d.index is not None else torch.cuda.current_device()) != self._ctx_device:
                return 0
        return int(_lib.bsrnn_workspace_rows(self._ctx))

    def evaluate(self, mix, speech, return_estimate=False):
        """The reference's validation arithmetic on the device (m_dataset.py:182-226 `infer` + `train_infer` without
        the discriminator, and the "Separation dB" of infer.py:44-47): mix, speech [R, n] -> dict of
        loss / sdr / input_sdr / sisdr / l1_time / l1_re / l1_im / separation_db (see include/bsrnn_hip.h)."""
        if mix.dim() != 2 or tuple(mix.shape) != tuple(speech.shape):
            raise ValueError("expected mix and speech [R, n] of the same shape, got %s and %s" % (tuple(mix.shape), tuple(speech.shape)))
        dev = self._device_for(mix)
        m, s = self._prep(mix, dev), self._prep(speech, dev)
        R, n = m.shape
        vals = (ctypes.c_double * len(_native.METRIC_NAMES))()
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            est = torch.empty((R, (n // _spec.HOP) * _spec.HOP), device=dev, dtype=torch.float32) if return_estimate else None
            _check(_lib.bsrnn_evaluate(ctx, _ptr(m), _ptr(s), R, n, _ptr(est) if return_estimate else None, vals, _stream_ptr(dev)))
        out = {k: vals[i] for i, k in enumerate(_native.METRIC_NAMES)}
        if return_estimate:
            out["x_time"] = est if mix.is_cuda else est.cpu()
        return out

    def evaluate_ragged(self, mix, speech, lengths, clip_rows=None, return_estimate=False):
        """`evaluate` for clips of different lengths in one call: mix, speech [R, n_max]; clip c owns clip_rows[c] consecutive rows (None:
        one row per clip) of lengths[c] samples each, 1024 < lengths[c] <= n_max; what lies behind a row's samples is never read.  Returns
        a list of dicts, one per clip, each what `evaluate` gives for that clip alone (to rounding): a clip is the unit of the reference's
        metrics, nothing is summed across clips (include/bsrnn_hip.h, bsrnn_evaluate_ragged).  With return_estimate each dict also has
        "x_time": the clip's rows cut to its own (n // 1024) * 1024 samples."""
        return self._evaluate_clips("evaluate_ragged", mix, speech, lengths, clip_rows, return_estimate, None)

    def evaluate_long_ragged(self, mix, speech, lengths, clip_rows=None, segment_frames=256, return_estimate=False):
        """`evaluate_ragged` in segments, for clips that are long AND unequal: arguments, checks and result as `evaluate_ragged`, each clip's
        numbers what `evaluate` gives for that clip alone (to rounding), from a workspace of R * segment_frames frame rows and - without
        return_estimate - an estimate buffer of one segment: nothing grows with the clips' length.  The separation is
        `separate_long_ragged`'s, so put the clips LONGEST FIRST; segment_frames is checked as there, and segment_frames >= Tmax is
        `evaluate_ragged` itself (bit-identical).  The sums are formed segment by segment and the SI-SDR from the rows' totals
        (include/bsrnn_hip.h, bsrnn_evaluate_long_ragged)."""
        return self._evaluate_clips("evaluate_long_ragged", mix, speech, lengths, clip_rows, return_estimate, segment_frames)

    def evaluate_long(self, mix, speech, segment_frames=256, return_estimate=False):
        """`evaluate` for one clip of any length in bounded memory: mix, speech [R, n] -> the dict of `evaluate`, through
        `evaluate_long_ragged` with the R rows as one clip."""
        if (not isinstance(mix, torch.Tensor) or not isinstance(speech, torch.Tensor) or mix.dim() != 2
                or tuple(mix.shape) != tuple(speech.shape) or mix.shape[0] < 1):
            raise ValueError("evaluate_long: expected mix and speech [R, n] of the same shape, got %s and %s" % (
                tuple(mix.shape) if isinstance(mix, torch.Tensor) else type(mix).__name__,
                tuple(speech.shape) if isinstance(speech, torch.Tensor) else type(speech).__name__))
        return self._evaluate_clips("evaluate_long", mix, speech, [mix.shape[1]], [mix.shape[0]], return_estimate, segment_frames)[0]

    def _evaluate_clips(self, who, mix, speech, lengths, clip_rows, return_estimate, segment_frames):
        """The ragged evaluate calls: checks first, then bsrnn_evaluate_ragged (who = "evaluate_ragged": no segments) or
        bsrnn_evaluate_long_ragged."""
        if (not isinstance(mix, torch.Tensor) or not isinstance(speech, torch.Tensor) or mix.dim() != 2
                or tuple(mix.shape) != tuple(speech.shape)):
            raise ValueError(who + ": expected mix and speech [R, n_max] of the same shape, got %s and %s" % (
                tuple(mix.shape) if isinstance(mix, torch.Tensor) else type(mix).__name__,
                tuple(speech.shape) if isinstance(speech, torch.Tensor) else type(speech).__name__))
        R, n_max = mix.shape
        try:
            lens = [int(x) for x in lengths]
            rows = [1] * len(lens) if clip_rows is None else [int(x) for x in clip_rows]
        except TypeError:
            raise ValueError(who + ": lengths and clip_rows must be sequences of ints") from None
        if not lens or len(rows) != len(lens):
            raise ValueError(who + ": %d lengths and %d row counts, need one of each per clip and at least one clip" % (len(lens), len(rows)))
        for c, (n, ch) in enumerate(zip(lens, rows)):
            if ch < 1:
                raise ValueError(who + ": clip %d has %d rows, need at least 1" % (c, ch))
            if not _spec.HOP < n <= n_max:
                raise ValueError(who + ": clip %d has %d samples, need 1024 < length <= %d" % (c, n, n_max))
        seg = None
        if who != "evaluate_ragged":
            try:
                seg = int(segment_frames)
            except (TypeError, ValueError):
                raise ValueError(who + ": segment_frames must be an int, got %r" % (segment_frames,)) from None
            if seg < 1:
                raise ValueError(who + ": segment_frames = %d (at least one frame per segment)" % seg)
        if sum(rows) != R:
            raise ValueError(who + ": the clips own %d rows, mix has %d" % (sum(rows), R))
        dev = self._device_for(mix)
        m, s = self._prep(mix, dev), self._prep(speech, dev)
        n_clips = len(lens)
        vals = (ctypes.c_double * (n_clips * len(_native.METRIC_NAMES)))()
        with torch.cuda.device(dev):
            ctx = self._context(dev)
            est = torch.empty((R, (max(lens) // _spec.HOP) * _spec.HOP), device=dev, dtype=torch.float32) if return_estimate else None
            head = (ctx, _ptr(m), _ptr(s), n_max, (ctypes.c_int64 * n_clips)(*lens), (ctypes.c_int32 * n_clips)(*rows), n_clips)
            tail = (_ptr(est) if return_estimate else None, vals, _stream_ptr(dev))
            if seg is None:
                _check(_lib.bsrnn_evaluate_ragged(*head, *tail))
            else:
                _check(_lib.bsrnn_evaluate_long_ragged(*head, seg, *tail))
        out, r0, nm = [], 0, len(_native.METRIC_NAMES)
        for c, (n, ch) in enumerate(zip(lens, rows)):
            d = {k: vals[c * nm + i] for i, k in enumerate(_native.METRIC_NAMES)}
            if return_estimate:
                x = est[r0:r0 + ch, :(n // _spec.HOP) * _spec.HOP].contiguous()
                d["x_time"] = x if mix.is_cuda else x.cpu()
            out.append(d)
            r0 += ch
        return out

    def evaluate_many(self, pairs, max_rows=64, max_padding=0.25):
        """`evaluate` for a list of (mix, speech) pairs of different lengths, batched: each tensor [n] or [ch, n] (n > 1024), both of a pair
        of the same rank and channel count and cut to their common length.  `spec.ragged_buckets` groups the pairs exactly as
        `separate_many` groups clips; each bucket is packed into two [rows, n_max] buffers and runs as ONE `evaluate_ragged` call.
        Returns the per-pair metric dicts in input order."""
        return self._evaluate_pairs("evaluate_many", pairs, lambda frames, rows: _spec.ragged_buckets(frames, rows, max_rows, max_padding),
                                    self.evaluate_ragged)

    def evaluate_many_long(self, pairs, segment_frames=256, max_rows=64):
        """`evaluate_many` for pairs that are long and of very different lengths: pairs as `evaluate_many` takes them.  `spec.long_buckets`
        sorts them longest first and fills buckets of at most `max_rows` rows - no padding cap, the segments bound the padding - and each
        bucket runs as ONE `evaluate_long_ragged` call, rows longest first.  Returns the per-pair metric dicts in input order."""
        try:
            seg = int(segment_frames)
        except (TypeError, ValueError):
            raise ValueError("evaluate_many_long: segment_frames must be an int, got %r" % (segment_frames,)) from None
        if seg < 1:
            raise ValueError("evaluate_many_long: segment_frames = %d (at least one frame per segment)" % seg)
        return self._evaluate_pairs("evaluate_many_long", pairs, lambda frames, rows: _spec.long_buckets(frames, rows, max_rows),
                                    lambda m, s, lens, rows: self.evaluate_long_ragged(m, s, lens, rows, seg))

    def _evaluate_pairs(self, who, pairs, buckets_of, run):
        """The batched evaluate calls: the pairs checked, grouped by buckets_of(frames, rows), each bucket packed and handed to run."""
        pairs = list(pairs)
        shapes = []
        for i, p in enumerate(pairs):
            ok = isinstance(p, (tuple, list)) and len(p) == 2 and all(isinstance(t, torch.Tensor) and t.dim() in (1, 2) for t in p)
            ok = ok and p[0].dim() == p[1].dim() and (p[0].dim() == 1 or (p[0].shape[0] == p[1].shape[0] and p[0].shape[0] >= 1))
            n = min(p[0].shape[-1], p[1].shape[-1]) if ok else 0
            if not ok or n <= _spec.HOP:
                raise ValueError("%s: pair %d must be (mix, speech) tensors, both [n] or both [ch, n], with n > 1024" % (who, i))
            shapes.append((1 if p[0].dim() == 1 else p[0].shape[0], n))
        buckets = buckets_of([_spec.n_frames(n) for _, n in shapes], [ch for ch, _ in shapes])
        if not pairs:
            return []
        dev = next((t.device for p in pairs for t in p if t.is_cuda), None) or self._device_for(pairs[0][0])
        results = [None] * len(pairs)
        for bucket in buckets:
            rows = [shapes[i][0] for i in bucket]
            lens = [shapes[i][1] for i in bucket]
            bufs = torch.empty((2, sum(rows), max(lens)), device=dev, dtype=torch.float32)    # (behind a row's end nothing is read)
            r0 = 0
            for i, ch, n in zip(bucket, rows, lens):
                for k in range(2):
                    bufs[k, r0:r0 + ch, :n] = pairs[i][k].detach().reshape(ch, -1)[:, :n].to(device=dev, dtype=torch.float32)
                r0 += ch
            for i, d in zip(bucket, run(bufs[0], bufs[1], lens, rows)):
                results[i] = d
        return results

    # ------------------------------------------------------------------ measurement
    def set_profiling(self, on, device=None):
        """on: False/True (all stages) or an iterable of stage names to bracket with events."""
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if on is True:
            mask = -1
        elif not on:
            mask = 0
        else:
            names = _native.stage_names()
            mask = 0
            for s in on:
                mask |= 1 << names.index(s)
        _check(_lib.bsrnn_set_profiling(self._context(dev), mask))

    def stage_times(self, reset=True):
        """-> {stage: (total_ms, launches)} accumulated while profiling was on."""
        n = _lib.bsrnn_stage_count()
        ms = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        _check(_lib.bsrnn_stage_times(self._ctx, ms, cnt, 1 if reset else 0))
        return {name: (ms[i], cnt[i]) for i, name in enumerate(_native.stage_names())}

    def save_flat(self, path):
        from . import weights
        weights.save_flat(path, {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}, self.band_widths)


class StreamingSeparator:
    """Device-resident form of the infer-streaming.py loop (lines 84-147): feed [C, 1024] chunks,
    get [C, 1024] chunks delayed by one hop.  State, the sliding buffer and the previous
    synthesis frame stay on the GPU between steps."""

    def __init__(self, model, channels=2, device=None):
        self.model = model
        self.C = channels
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        ctx = model._context(self.device)
        h = ctypes.c_void_p()
        _check(_lib.bsrnn_stream_create(ctx, channels, ctypes.byref(h)))
        self._h = h
        self._steps = 0
        self._pending = None        # process(): the samples (fewer than one hop) that wait for the next call, on the device

    def __del__(self):
        try:
            _lib.bsrnn_stream_destroy(self._h)
        except Exception:
            pass

    def reset(self):
        _check(_lib.bsrnn_stream_reset(self._h, _stream_ptr(self.device)))
        self._pending = None

    def reserve(self, max_hops):
        """Do now what a later process() of up to max_hops hops would otherwise do at first use (workspace, task tables,
        kernel loading): such calls then allocate nothing."""
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_stream_reserve(self._h, int(max_hops)))

    def process(self, wave, mix=1.0):
        """wave [C, n] float32 (cuda or cpu), any n >= 0 -> [C, L*1024] on the same device: what L consecutive step() calls
        return, from one library call (bsrnn_stream_process).  L = (pending + n) // 1024; a remainder of fewer than 1024
        samples stays on the device and is prepended to the next call.  Carries on from and for step() in any mixture."""
        if wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("expected wave [%d, n], got %s" % (self.C, tuple(wave.shape)))
        # the same look at the model's parameters as step() takes (see there), once per call
        if self._steps % 32 == 0 or self.model._weights_touched(self._steps):
            self.model._plist = None
            with torch.cuda.device(self.device):
                self.model._context(self.device)
        self._steps += 1
        w = wave.detach().to(device=self.device, dtype=torch.float32)
        if self._pending is not None and self._pending.shape[1]:
            w = torch.cat((self._pending, w), 1)
        L = w.shape[1] // _spec.HOP
        self._pending = w[:, L * _spec.HOP:].clone()
        if L == 0:
            return torch.empty((self.C, 0), dtype=torch.float32, device=wave.device)
        x = w[:, :L * _spec.HOP].contiguous()
        out = torch.empty_like(x)
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_stream_process(self._h, _ptr(x), _ptr(out), L, float(mix), _stream_ptr(self.device)))
        return out if wave.is_cuda else out.cpu()

    def step(self, chunk, mix=1.0):
        """chunk [C, 1024] float32 (cuda or cpu) -> same-shaped output on the same device."""
        if tuple(chunk.shape) != (self.C, _spec.HOP):
            raise ValueError("expected chunk [%d, 1024], got %s" % (self.C, tuple(chunk.shape)))
        # The reference's forward_recurrent always sees the current parameters (bsrnn.py:445).  Here the weights live packed on the
        # device, so a running stream looks at the model every step, cheaply: a rotating eighth of the parameters' version counters
        # and storage pointers per step (an optimizer step or load_state_dict is seen at the next chunk, an in-place edit or
        # rebinding of a single tensor within 8 chunks), and the whole module tree again every 32nd step (a parameter OBJECT
        # swapped into a submodule).  model.refresh_weights() forces it at once.
        if self._steps % 32 == 0 or self.model._weights_touched(self._steps):
            self.model._plist = None            # (re-read the parameter objects and their storage pointers)
            with torch.cuda.device(self.device):
                self.model._context(self.device)
        self._steps += 1
        if chunk.is_cuda:
            c = chunk.detach().to(torch.float32).contiguous()
            out = torch.empty_like(c)
            with torch.cuda.device(self.device):
                _check(_lib.bsrnn_stream_step(self._h, _ptr(c), _ptr(out), float(mix), _stream_ptr(self.device)))
            return out
        c = np.ascontiguousarray(chunk.detach().numpy(), dtype=np.float32)
        o = np.empty_like(c)
        _check(_lib.bsrnn_stream_step_host(self._h, c.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p), float(mix)))
        return torch.from_numpy(o)

    def state(self):
        K = len(self.model.band_widths)
        s = np.empty((4, 2, self.C * K, band_features), np.float32)
        _check(_lib.bsrnn_stream_get_state(self._h, s.ctypes.data_as(ctypes.c_void_p)))
        return torch.from_numpy(s)

    # ------------------------------------------------------------------ rows that live apart (session slots)
    def _look_at_weights(self):
        # the same look at the model's parameters as step() takes (see there), once per call
        if self._steps % 32 == 0 or self.model._weights_touched(self._steps):
            self.model._plist = None
            with torch.cuda.device(self.device):
                self.model._context(self.device)
        self._steps += 1

    def _check_row(self, row, what):
        if isinstance(row, bool) or not isinstance(row, (int, np.integer)):
            raise ValueError("%s: row must be an int, got %s" % (what, type(row).__name__))
        if not 0 <= row < self.C:
            raise ValueError("%s: row %d is outside [0, %d)" % (what, row, self.C))
        return int(row)

    def row_floats(self):
        """Floats of one row's carry as get_row / set_row move it: buf[2048], prev[2048], state[4][2][K][64]."""
        return 2 * _spec.N_FFT + 8 * len(self.model.band_widths) * band_features

    def process_rows(self, wave, active=None, mix=1.0):
        """wave [C, L*1024] float32 (cuda or cpu), whole hops -> [C, L*1024] on the same device (bsrnn_stream_process_rows): rows with a
        true entry in `active` (a sequence or tensor of C flags; None: every row) take the L hops exactly as process() would give them,
        the others are HELD - their carry stays bit for bit, their output rows are zeros and their input rows are never read.  `mix` is
        one wet / dry value or a [C] tensor of one per row.  Takes no part in process()'s carrying of partial hops."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("process_rows: expected wave [%d, L*1024], got %s" % (
                self.C, tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__))
        if wave.shape[1] % _spec.HOP:
            raise ValueError("process_rows: wave must hold whole hops of 1024 samples, got %d samples per row" % wave.shape[1])
        flags = None
        if active is not None:
            try:
                flags = [bool(a) for a in (active.tolist() if isinstance(active, (torch.Tensor, np.ndarray)) else active)]
            except TypeError:
                raise ValueError("process_rows: active must be a sequence of %d flags, got %s" % (self.C, type(active).__name__)) from None
            if len(flags) != self.C:
                raise ValueError("process_rows: %d flags for %d rows" % (len(flags), self.C))
        mix_rows = None
        if isinstance(mix, torch.Tensor):
            if tuple(mix.shape) != (self.C,):
                raise ValueError("process_rows: mix must be a float or a tensor [%d], got %s" % (self.C, tuple(mix.shape)))
            mix_rows, mix = mix, 1.0
        elif isinstance(mix, bool) or not isinstance(mix, (int, float, np.floating, np.integer)):
            raise ValueError("process_rows: mix must be a float or a tensor [%d], got %s" % (self.C, type(mix).__name__))
        L = wave.shape[1] // _spec.HOP
        if L == 0:
            return torch.empty((self.C, 0), dtype=torch.float32, device=wave.device)
        self._look_at_weights()
        x = wave.detach().to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        if mix_rows is not None:
            mix_rows = mix_rows.detach().to(device=self.device, dtype=torch.float32).contiguous()
        act = (ctypes.c_uint8 * self.C)(*flags) if flags is not None else None
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_stream_process_rows(self._h, _ptr(x), _ptr(out), L, act, _ptr(mix_rows) if mix_rows is not None else None,
                                                  float(mix), _stream_ptr(self.device)))
        return out if wave.is_cuda else out.cpu()

    def process_hops(self, wave, hops, mix=1.0):
        """wave [C, L*1024] float32 (cuda or cpu), whole hops, and hops, a sequence or tensor of C ints in [0, L] -> [C, L*1024] on the same
        device, from one library call (bsrnn_stream_process_hops): row r takes its first hops[r] hops exactly as that many step() calls
        would give them, its output row is zeros behind them, its input row is never read behind them, and its carry is the one after
        hops[r] hops; a row at 0 is held as by process_rows.  At most 255 hops per call.  `mix` is one wet / dry value or a [C] tensor
        of one per row.  Takes no part in process()'s carrying of partial hops."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("process_hops: expected wave [%d, L*1024], got %s" % (
                self.C, tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__))
        if wave.shape[1] % _spec.HOP:
            raise ValueError("process_hops: wave must hold whole hops of 1024 samples, got %d samples per row" % wave.shape[1])
        L = wave.shape[1] // _spec.HOP
        if L > _native.STREAM_HOPS_MAX:
            raise ValueError("process_hops: %d hops, a call takes at most %d" % (L, _native.STREAM_HOPS_MAX))
        try:
            counts = list(hops.tolist() if isinstance(hops, (torch.Tensor, np.ndarray)) else hops)
        except TypeError:
            raise ValueError("process_hops: hops must be a sequence of %d ints, got %s" % (self.C, type(hops).__name__)) from None
        if len(counts) != self.C:
            raise ValueError("process_hops: %d counts for %d rows" % (len(counts), self.C))
        for r, h in enumerate(counts):
            if isinstance(h, bool) or not isinstance(h, (int, np.integer)):
                raise ValueError("process_hops: the count of row %d must be an int, got %s" % (r, type(h).__name__))
            if not 0 <= h <= L:
                raise ValueError("process_hops: row %d has %d hops, outside [0, %d]" % (r, h, L))
        mix_rows = None
        if isinstance(mix, torch.Tensor):
            if tuple(mix.shape) != (self.C,):
                raise ValueError("process_hops: mix must be a float or a tensor [%d], got %s" % (self.C, tuple(mix.shape)))
            mix_rows, mix = mix, 1.0
        elif isinstance(mix, bool) or not isinstance(mix, (int, float, np.floating, np.integer)):
            raise ValueError("process_hops: mix must be a float or a tensor [%d], got %s" % (self.C, type(mix).__name__))
        if L == 0:
            return torch.empty((self.C, 0), dtype=torch.float32, device=wave.device)
        self._look_at_weights()
        x = wave.detach().to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        if mix_rows is not None:
            mix_rows = mix_rows.detach().to(device=self.device, dtype=torch.float32).contiguous()
        cnt = (ctypes.c_int32 * self.C)(*[int(h) for h in counts])
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_stream_process_hops(self._h, _ptr(x), _ptr(out), L, cnt, _ptr(mix_rows) if mix_rows is not None else None,
                                                  float(mix), _stream_ptr(self.device)))
        return out if wave.is_cuda else out.cpu()

    def reset_rows(self, rows):
        """Zero the carry of the listed rows (bsrnn_stream_reset_rows): each then continues as the same row of a fresh stream would."""
        try:
            rows = [self._check_row(r, "reset_rows") for r in rows]
        except TypeError:
            raise ValueError("reset_rows: rows must be a sequence of ints, got %s" % type(rows).__name__) from None
        if not rows:
            raise ValueError("reset_rows: no rows")
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_stream_reset_rows(self._h, (ctypes.c_int32 * len(rows))(*rows), len(rows), _stream_ptr(self.device)))

    def get_row(self, row):
        """One row's carry as a CPU tensor [row_floats()] (bsrnn_stream_get_row; synchronous)."""
        row = self._check_row(row, "get_row")
        blob = np.empty(self.row_floats(), np.float32)
        _check(_lib.bsrnn_stream_get_row(self._h, row, blob.ctypes.data_as(ctypes.c_void_p)))
        return torch.from_numpy(blob)

    def set_row(self, row, blob):
        """Put a carry taken with get_row - from this stream or another one of the same C and band table - into `row`: the row continues
        bit for bit as it would have where it came from (bsrnn_stream_set_row; synchronous)."""
        row = self._check_row(row, "set_row")
        if not isinstance(blob, torch.Tensor) or blob.numel() != self.row_floats() or blob.dim() != 1:
            raise ValueError("set_row: blob must be a tensor [%d], got %s" % (
                self.row_floats(), tuple(blob.shape) if isinstance(blob, torch.Tensor) else type(blob).__name__))
        b = np.ascontiguousarray(blob.detach().to("cpu", torch.float32).numpy())
        _check(_lib.bsrnn_stream_set_row(self._h, row, b.ctypes.data_as(ctypes.c_void_p)))


def resample_len(n_in, rate_in, rate_out):
    """Samples bsrnn_resample gives for n_in: ceil(n_in * up / down).  ValueError for what the library refuses (a rate < 1, a reduced
    max(up, down) beyond 1024, n_in < 1)."""
    n = _lib.bsrnn_resample_len(int(n_in), int(rate_in), int(rate_out))
    if n < 0:
        raise ValueError("resample: cannot convert %s samples from %s to %s Hz (rates >= 1, reduced max(up, down) <= 1024, n >= 1)" % (
            n_in, rate_in, rate_out))
    return n


class Resampler:
    """Streaming sample-rate conversion on the device (bsrnn_resampler_*): feed blocks of any length, get the output samples that have
    become determined; flush() gives the rest.  The concatenation equals model.resample() of the concatenated input, value for value.
    Replaces the host-side audio.resample in front of a streaming loop (infer-streaming.py --device-resample)."""

    def __init__(self, model, channels, rate_in, rate_out):
        resample_len(1, rate_in, rate_out)          # (the limits, as a ValueError)
        self.model = model
        self.C = int(channels)
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.device = torch.device("cuda", model._ctx_device if model._ctx_device is not None else torch.cuda.current_device())
        with torch.cuda.device(self.device):
            ctx = model._context(self.device)
            h = ctypes.c_void_p()
            _check(_lib.bsrnn_resampler_create(ctx, self.C, self.rate_in, self.rate_out, ctypes.byref(h)))
        self._h = h
        self._taken = self._given = 0       # the library's two counters, mirrored to size flush()'s result before the call

    def __del__(self):
        try:
            _lib.bsrnn_resampler_destroy(self._h)
        except Exception:
            pass

    def ready(self, n_in):
        """Samples per row the next process() of n_in samples would return."""
        return int(_lib.bsrnn_resampler_ready(self._h, int(n_in)))

    def process(self, wave):
        """wave [C, n] float32 on the resampler's device, any n >= 0 -> [C, ready(n)]."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("Resampler.process: expected wave [C = %d, n], got %s" % (
                self.C, tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__))
        if wave.dtype != torch.float32 or wave.device != self.device:
            raise ValueError("Resampler.process: expected a float32 tensor on %s, got %s on %s" % (self.device, wave.dtype, wave.device))
        n = ctypes.c_int64(-1)
        w, w_stride = BSRNN._rows_view(wave.detach())
        with torch.cuda.device(self.device):
            out = torch.empty((self.C, self.ready(w.shape[1])), device=self.device, dtype=torch.float32)
            _check(_lib.bsrnn_resampler_process(self._h, _ptr(w), w_stride, w.shape[1], _ptr(out), out.shape[1], ctypes.byref(n),
                                                _stream_ptr(self.device)))
        assert n.value == out.shape[1], (n.value, tuple(out.shape))
        self._taken += w.shape[1]
        self._given += out.shape[1]
        return out

    def flush(self):
        """The samples still owed for the input so far (the future counting as zeros); the resampler starts afresh."""
        owed = (resample_len(self._taken, self.rate_in, self.rate_out) if self._taken else 0) - self._given
        n = ctypes.c_int64(-1)
        with torch.cuda.device(self.device):
            out = torch.empty((self.C, owed), device=self.device, dtype=torch.float32)
            _check(_lib.bsrnn_resampler_flush(self._h, _ptr(out), owed, ctypes.byref(n), _stream_ptr(self.device)))
        assert n.value == owed, (n.value, owed)
        self._taken = self._given = 0
        return out

    def reset(self):
        _check(_lib.bsrnn_resampler_reset(self._h, _stream_ptr(self.device)))
        self._taken = self._given = 0


def _check_pairs(pairs, who):
    """[(rate_in, rate_out), ...] as ints, or ValueError for what bsrnn_resampler_bank_create refuses (no device needed)."""
    try:
        pairs = [(int(a), int(b)) for a, b in pairs]
    except (TypeError, ValueError):
        raise ValueError("%s: pairs must be a sequence of (rate_in, rate_out), got %r" % (who, pairs)) from None
    if not 1 <= len(pairs) <= _native.BANK_PAIRS_MAX:
        raise ValueError("%s: %d rate pairs, a bank takes 1 to %d" % (who, len(pairs), _native.BANK_PAIRS_MAX))
    for a, b in pairs:
        resample_len(1, a, b)
    return pairs


class ResamplerBank:
    """Streaming sample-rate conversion for rows that do NOT share a rate or a clock (bsrnn_resampler_bank_*): every row sits on one of
    the declared `pairs` [(rate_in, rate_out), ...] (at most 16), at its own place in its own stream, and one process() converts whatever
    each row brings - in one launch-bound library call.  Row r equals a one-row Resampler of r's pair value for value.  All rows start
    on pairs[0]."""

    def __init__(self, model, channels, pairs):
        self.pairs = _check_pairs(pairs, "ResamplerBank")
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or channels < 1:
            raise ValueError("ResamplerBank: channels must be a positive int, got %r" % (channels,))
        self.model = model
        self.C = int(channels)
        self.device = torch.device("cuda", model._ctx_device if model._ctx_device is not None else torch.cuda.current_device())
        n = len(self.pairs)
        with torch.cuda.device(self.device):
            ctx = model._context(self.device)
            h = ctypes.c_void_p()
            _check(_lib.bsrnn_resampler_bank_create(ctx, self.C, (ctypes.c_int32 * n)(*[p[0] for p in self.pairs]),
                                                    (ctypes.c_int32 * n)(*[p[1] for p in self.pairs]), n, ctypes.byref(h)))
        self._h = h
        # the library's per-row counters and pairs, mirrored to size the results before the calls
        self._taken, self._given, self._pair = [0] * self.C, [0] * self.C, [0] * self.C
        self._ratio = []                    # per pair: up, down, half (csrc/resample_host.h, resample_ratio)
        for a, b in self.pairs:
            g = math.gcd(a, b)
            self._ratio.append((b // g, a // g, 10 * max(a // g, b // g)))

    def __del__(self):
        try:
            _lib.bsrnn_resampler_bank_destroy(self._h)
        except Exception:
            pass

    def _rows(self, rows, who):
        try:
            rows = list(rows)
        except TypeError:
            raise ValueError("ResamplerBank.%s: rows must be a sequence of ints, got %s" % (who, type(rows).__name__)) from None
        for r in rows:
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)):
                raise ValueError("ResamplerBank.%s: a row must be an int, got %s" % (who, type(r).__name__))
            if not 0 <= r < self.C:
                raise ValueError("ResamplerBank.%s: row %d is outside [0, %d)" % (who, r, self.C))
        if len(set(rows)) != len(rows):
            raise ValueError("ResamplerBank.%s: a row is listed twice in %s" % (who, rows))
        return [int(r) for r in rows], (ctypes.c_int32 * len(rows))(*rows)

    def pair_of(self, row):
        return self._pair[self._rows([row], "pair_of")[0][0]]

    def assign(self, rows, pair):
        """The listed rows move to pairs[pair] and start a new stream there (host only)."""
        if isinstance(pair, bool) or not isinstance(pair, (int, np.integer)) or not 0 <= pair < len(self.pairs):
            raise ValueError("ResamplerBank.assign: pair %r is outside [0, %d)" % (pair, len(self.pairs)))
        rows, arr = self._rows(rows, "assign")
        _check(_lib.bsrnn_resampler_bank_assign(self._h, arr, len(rows), int(pair)))
        for r in rows:
            self._taken[r] = self._given[r] = 0
            self._pair[r] = int(pair)

    def reset_rows(self, rows):
        """The listed rows forget their stream so far and start a new one on the pair they have (host only)."""
        rows, arr = self._rows(rows, "reset_rows")
        _check(_lib.bsrnn_resampler_bank_reset_rows(self._h, arr, len(rows)))
        for r in rows:
            self._taken[r] = self._given[r] = 0

    def ready(self, row, n):
        """Samples the next process() would return for `row` if it gave the row n samples."""
        row = self._rows([row], "ready")[0][0]
        return int(_lib.bsrnn_resampler_bank_ready(self._h, row, int(n)))

    def _ready(self, r, n):
        # ready() from the mirrored counters, without a library call per row: the outputs whose last input, floor((j * down + half) / up),
        # has arrived (csrc/resample_host.h, resample_ready).  process() holds the library's own counts against it.
        up, down, half = self._ratio[self._pair[r]]
        N = self._taken[r] + n
        a = N * up - half - 1
        return (0 if N < 1 or a < 0 else min(a // down + 1, -(-N * up // down))) - self._given[r]

    def process(self, wave, counts):
        """wave [C, n] float32 on the bank's device and counts, C ints in [0, n] -> (tensor [C, max count out], the counts out as a list):
        row r reads its first counts[r] samples and nothing behind them, and gets the outputs that have become determined in
        out[r, :counts_out[r]]; what lies behind them in the tensor is unspecified.  A count of 0 holds the row."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("ResamplerBank.process: expected wave [C = %d, n], got %s" % (
                self.C, tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__))
        if wave.dtype != torch.float32 or wave.device != self.device:
            raise ValueError("ResamplerBank.process: expected a float32 tensor on %s, got %s on %s" % (self.device, wave.dtype, wave.device))
        try:
            counts = list(counts.tolist() if isinstance(counts, (torch.Tensor, np.ndarray)) else counts)
        except TypeError:
            raise ValueError("ResamplerBank.process: counts must be a sequence of %d ints, got %s" % (self.C, type(counts).__name__)) from None
        if len(counts) != self.C:
            raise ValueError("ResamplerBank.process: %d counts for %d rows" % (len(counts), self.C))
        for r, n in enumerate(counts):
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
                raise ValueError("ResamplerBank.process: the count of row %d must be an int, got %s" % (r, type(n).__name__))
            if not 0 <= n <= wave.shape[1]:
                raise ValueError("ResamplerBank.process: row %d has %d samples, outside [0, %d]" % (r, n, wave.shape[1]))
        w, w_stride = BSRNN._rows_view(wave.detach())
        want = [self._ready(r, n) if n else 0 for r, n in enumerate(counts)]
        n_in = (ctypes.c_int64 * self.C)(*[int(n) for n in counts])
        n_out = (ctypes.c_int64 * self.C)(*([-1] * self.C))
        with torch.cuda.device(self.device):
            out = torch.empty((self.C, max(want)), device=self.device, dtype=torch.float32)
            _check(_lib.bsrnn_resampler_bank_process(self._h, _ptr(w), w_stride, n_in, _ptr(out), out.shape[1], n_out, _stream_ptr(self.device)))
        got = list(n_out)
        assert got == want, (got, want)
        for r in range(self.C):
            self._taken[r] += int(counts[r])
            self._given[r] += got[r]
        return out, got

    def flush_rows(self, rows):
        """The listed rows get the samples they are still owed for their input so far (the future counting as zeros) and start afresh;
        the others are untouched.  -> (tensor [C, max count], the counts as a list: 0 for rows not listed)."""
        rows, arr = self._rows(rows, "flush_rows")
        want = [0] * self.C
        for r in rows:
            want[r] = (resample_len(self._taken[r], *self.pairs[self._pair[r]]) if self._taken[r] else 0) - self._given[r]
        n_out = (ctypes.c_int64 * self.C)(*([-1] * self.C))
        with torch.cuda.device(self.device):
            out = torch.empty((self.C, max(want)), device=self.device, dtype=torch.float32)
            _check(_lib.bsrnn_resampler_bank_flush_rows(self._h, arr, len(rows), _ptr(out), out.shape[1], n_out, _stream_ptr(self.device)))
        got = list(n_out)
        assert got == want, (got, want)
        for r in rows:
            self._taken[r] = self._given[r] = 0
        return out, got


class _StreamPoolType(type):
    """StreamPool(model, slots, rows_per_session=1, device=None, rates=None): the keyword `rates` is taken HERE, by the call of the
    class, and checked before anything else happens; StreamPool.__init__ keeps the four parameters it has always had, which callers
    and tests/test_stream_rows_host.py hold it to (inspect.signature(StreamPool) shows the whole call)."""

    def __call__(cls, model, slots, rows_per_session=1, device=None, rates=None):
        rates = cls._checked_rates(rates)
        pool = super().__call__(model, slots, rows_per_session, device)
        pool.rates = rates
        return pool


class StreamPool(metaclass=_StreamPoolType):
    """Many live sessions on one wide stream: `slots` sessions of `rows_per_session` rows each share one StreamingSeparator of
    slots * rows_per_session rows, and one step() serves whichever of them have audio this tick at the price of one streaming call
    (a step is launch-bound: its cost hardly grows with the rows).  feed() does the same for sessions that do NOT deliver audio in lock
    step: each gives whatever it has, and one call advances every session by its own number of hops.  Sessions join (open), leave
    (close), pause (not named in a step or feed: their rows are held) and move between pools (export / adopt) one by one.  The stream is created at the first call that needs the
    device; shape and type errors are raised before that.

    Sessions at their own sample rates: with `rates`, a tuple of at most 16 rates, open(sample_rate=r) makes a session that gives and
    gets audio at r, one of them.  feed() then converts what all such sessions bring to the model's 44.1 kHz in ONE call of a
    ResamplerBank (a rate pair, a count and a stream position per row), runs everybody's hops as before, and converts the separated
    audio back in one more; the stream's one-hop delay is taken out of such a session's audio (its first hop is dropped), so what it
    gets lines up with what it gave, and drain() ends its audio.  The two banks are made with the stream, and only when `rates` is
    given: without it the pool makes exactly the library calls it made before."""

    MODEL_RATE = 44100

    @classmethod
    def _checked_rates(cls, rates):
        """`rates` as a tuple of ints (None stays None), or ValueError for what the conversions to and from the model's rate refuse."""
        if rates is None:
            return None
        try:
            rates = tuple(rates)
        except TypeError:
            raise ValueError("StreamPool: rates must be a tuple of sample rates, got %s" % type(rates).__name__) from None
        if not 1 <= len(rates) <= _native.BANK_PAIRS_MAX:
            raise ValueError("StreamPool: %d rates, a pool takes 1 to %d" % (len(rates), _native.BANK_PAIRS_MAX))
        for r in rates:
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)):
                raise ValueError("StreamPool: a rate must be an int, got %r" % (r,))
            resample_len(1, r, cls.MODEL_RATE)          # (the limits of the conversion, as a ValueError)
        return tuple(int(r) for r in rates)

    def __init__(self, model, slots, rows_per_session=1, device=None):
        for name, v in (("slots", slots), ("rows_per_session", rows_per_session)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("StreamPool: %s must be a positive int, got %r" % (name, v))
        if slots * rows_per_session > _native.STREAM_ROWS_MAX:
            raise ValueError("StreamPool: %d slots x %d rows is more than the %d rows a rows call takes" % (slots, rows_per_session, _native.STREAM_ROWS_MAX))
        self.model, self.slots, self.rows, self._device = model, int(slots), int(rows_per_session), device
        self._st = None
        self._slot = {}                     # session id -> slot
        self._free = list(range(self.slots))
        self._next = 0
        self._pend = {}                     # feed(): session id -> the samples (fewer than one hop) that wait for its next feed
        self.rates = None                   # the pool's session rates; the call of the class sets them (_StreamPoolType)
        self._rate = {}                     # session id -> index into rates, for the sessions that have one
        self._skip = {}                     # such a session -> samples of the stream's delay still to be dropped from its output
        self._bank_in = self._bank_out = None

    def _stream(self):
        if self._st is None:
            self._st = StreamingSeparator(self.model, channels=self.slots * self.rows, device=self._device)
            if self.rates is not None:
                C = self.slots * self.rows
                self._bank_in = ResamplerBank(self.model, C, [(r, self.MODEL_RATE) for r in self.rates])
                self._bank_out = ResamplerBank(self.model, C, [(self.MODEL_RATE, r) for r in self.rates])
                for sid, k in self._rate.items():
                    self._bank_in.assign(list(self._rows_of(sid)), k)
                    self._bank_out.assign(list(self._rows_of(sid)), k)
        return self._st

    def _rows_of(self, sid):
        slot = self._slot[sid]              # KeyError: no such session
        return range(slot * self.rows, (slot + 1) * self.rows)

    def sessions(self):
        return list(self._slot)

    def open(self, sample_rate=None):
        """-> a new session's id; its rows start from silence.  sample_rate: None or the model's 44100 for a session that gives and gets
        audio at the model's rate, else one of the pool's `rates`.  ValueError when every slot is taken or the rate is not one of them."""
        k = None
        if sample_rate is not None and sample_rate != self.MODEL_RATE:
            if self.rates is None or sample_rate not in self.rates:
                raise ValueError("StreamPool.open: sample_rate %r is not one of the pool's rates %r" % (sample_rate, self.rates))
            k = self.rates.index(sample_rate)
        if not self._free:
            raise ValueError("StreamPool: all %d slots are in use" % self.slots)
        slot = self._free.pop(0)
        sid, self._next = self._next, self._next + 1
        self._slot[sid] = slot
        if self._st is not None:            # (a stream that does not exist yet starts zeroed)
            self._st.reset_rows(list(self._rows_of(sid)))
        if k is not None:
            self._rate[sid], self._skip[sid] = k, _spec.HOP
            if self._bank_in is not None:   # (banks that do not exist yet are told at their creation)
                self._bank_in.assign(list(self._rows_of(sid)), k)
                self._bank_out.assign(list(self._rows_of(sid)), k)
        return sid

    def close(self, sid):
        """The session leaves; samples of it that feed() kept waiting are dropped, and its rows of the resampler banks start afresh."""
        rows = list(self._rows_of(sid))
        if self._rate.pop(sid, None) is not None and self._bank_in is not None:
            self._bank_in.reset_rows(rows)
            self._bank_out.reset_rows(rows)
        self._skip.pop(sid, None)
        self._free.append(self._slot.pop(sid))
        self._free.sort()
        self._pend.pop(sid, None)

    def rate_of(self, sid):
        """The session's sample rate (44100 for one opened without)."""
        self._rows_of(sid)
        return self.rates[self._rate[sid]] if sid in self._rate else self.MODEL_RATE

    def pending(self, sid):
        """Samples per row of the session that wait for its next feed() (fewer than one hop) - at the MODEL's rate, 44.1 kHz, also for a
        session with a rate of its own: they are what the conversion has given and no whole hop has taken yet."""
        self._rows_of(sid)
        p = self._pend.get(sid)
        return 0 if p is None else int(p.shape[1])

    def feed(self, chunks, mix=None):
        """chunks {sid: tensor [rows_per_session, n]}, ANY n >= 0 and another one per session -> {sid: tensor [rows_per_session, h*1024] on
        its chunk's device}: every session advances by the h = (pending + n) // 1024 hops it has in hand, in ONE library call
        (bsrnn_stream_process_hops; several of at most 255 hops where a session brings more than that).  The remainder of fewer than one
        hop waits per session, on the device, and is prepended at the session's next feed, as StreamingSeparator.process does for a whole
        stream.  A session without a whole hop gets an empty tensor and its rows are held; so are sessions not named.  If nobody has a
        hop, no library call is made.  mix as in step().  The pending samples are NOT part of the carry that export() hands out: feed
        whole hops before moving a session, or move pending(sid) samples of its audio yourself.
        A session opened with a sample rate gives its chunk AT THAT RATE and gets back, at that rate, the output samples that have
        become determined - a length that varies from tick to tick, and lags what it gave by the two conversions' filters and the hop
        that is still filling; the stream's own one-hop delay is taken out.  All such sessions of a tick share one inbound and one
        outbound ResamplerBank call around the one bsrnn_stream_process_hops; drain() gives a session the rest."""
        if not isinstance(chunks, dict):
            raise ValueError("StreamPool.feed: chunks must be a dict {session id: tensor}, got %s" % type(chunks).__name__)
        for sid, t in chunks.items():
            self._rows_of(sid)
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != self.rows:
                raise ValueError("StreamPool.feed: session %r needs a tensor [%d, n], got %s" % (
                    sid, self.rows, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
        per_row = isinstance(mix, dict)
        if per_row:
            for sid, v in mix.items():
                self._rows_of(sid)
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError("StreamPool.feed: mix of session %r must be a float, got %s" % (sid, type(v).__name__))
        elif mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("StreamPool.feed: mix must be None, a float or a dict {session id: float}, got %s" % type(mix).__name__)
        rated = [sid for sid in chunks if sid in self._rate]
        if not rated:
            return self._feed_hops(chunks, mix)
        # Sessions with a rate: what they bring goes to 44.1 kHz in one bank call, then everybody's audio takes the path it always took,
        # then what came out for them goes back to their rates in one more
        self._stream()
        conv = self._bank_call(self._bank_in, {sid: chunks[sid] for sid in rated})
        res = self._feed_hops({sid: conv.get(sid, t) for sid, t in chunks.items()}, mix)
        back = self._bank_call(self._bank_out, {sid: self._undelayed(sid, res[sid]) for sid in rated})
        for sid in rated:
            res[sid] = back[sid] if chunks[sid].is_cuda else back[sid].cpu()
        return res

    def _undelayed(self, sid, out):
        """The stream's output for a session with a rate, without the samples of the one-hop delay that are still to be dropped."""
        k = min(self._skip[sid], out.shape[1])
        self._skip[sid] -= k
        return out[:, k:]

    def _bank_call(self, bank, blocks):
        """blocks {sid: tensor [rows_per_session, n]} of sessions with a rate -> {sid: tensor [rows_per_session, count] on the pool's
        device}, the samples that have become determined: ONE process() of the bank, every other row held.  The results are views of
        the call's one output tensor, which nobody else holds."""
        C = self.slots * self.rows
        dev = self._st.device
        n_max = max(t.shape[1] for t in blocks.values())
        if n_max == 0:
            return {sid: torch.empty((self.rows, 0), dtype=torch.float32, device=dev) for sid in blocks}
        wave = torch.empty((C, n_max), dtype=torch.float32, device=dev)
        counts = [0] * C
        for sid, t in blocks.items():
            rows = self._rows_of(sid)
            if t.shape[1]:
                wave[rows.start:rows.stop, :t.shape[1]] = t.detach().to(device=dev, dtype=torch.float32)
            for r in rows:
                counts[r] = t.shape[1]
        out, got = bank.process(wave, counts)
        res = {}
        for sid in blocks:
            rows = self._rows_of(sid)
            res[sid] = out[rows.start:rows.stop, :got[rows.start]]
        return res

    def _feed_hops(self, chunks, mix):
        """feed() behind its argument checks, for chunks at the model's rate."""
        per_row = isinstance(mix, dict)
        hop = _spec.HOP
        have = {sid: self.pending(sid) + t.shape[1] for sid, t in chunks.items()}
        anyone = any(n >= hop for n in have.values())
        # (the stream is made by the first feed that has a hop for it; until then what waits stays where the caller's tensors are)
        dev = self._stream().device if anyone else (self._st.device if self._st is not None else None)
        audio = {}
        for sid, t in chunks.items():
            w = t.detach().to(dtype=torch.float32) if dev is None else t.detach().to(device=dev, dtype=torch.float32)
            p = self._pend.get(sid)
            if p is not None and p.shape[1]:
                w = torch.cat((p.to(w.device), w), 1)
            audio[sid] = w
            self._pend[sid] = w[:, (have[sid] // hop) * hop:].clone()
        res = {sid: [] for sid in chunks}
        done = {sid: 0 for sid in chunks}
        C = self.slots * self.rows
        while any(have[sid] // hop > done[sid] for sid in chunks):
            st = self._st
            take = {sid: min(have[sid] // hop - done[sid], _native.STREAM_HOPS_MAX) for sid in chunks}
            L = max(take.values())
            wave = torch.zeros((C, L * hop), dtype=torch.float32, device=st.device)
            counts = [0] * C
            mix_rows = [1.0] * C
            for sid, h in take.items():
                rows = self._rows_of(sid)
                wave[rows.start:rows.stop, :h * hop] = audio[sid][:, done[sid] * hop:(done[sid] + h) * hop]
                for r in rows:
                    counts[r] = h
                    if per_row:
                        mix_rows[r] = float(mix.get(sid, 1.0))
            m = torch.tensor(mix_rows, dtype=torch.float32) if per_row else (1.0 if mix is None else float(mix))
            out = st.process_hops(wave, counts, m)
            for sid, h in take.items():
                rows = self._rows_of(sid)
                res[sid].append(out[rows.start:rows.stop, :h * hop])
                done[sid] += h
        ret = {}
        for sid, t in chunks.items():
            o = torch.cat(res[sid], 1) if res[sid] else torch.empty((self.rows, 0), dtype=torch.float32, device=t.device)
            ret[sid] = (o.clone() if len(res[sid]) == 1 else o) if t.is_cuda else o.cpu()
        return ret

    def step(self, chunks, mix=None):
        """chunks {sid: tensor [rows_per_session, L*1024]}, one L for all -> {sid: tensor of the same shape, on its chunk's device}, delayed
        by one hop like StreamingSeparator.step.  Sessions not named are held.  mix: None (1.0), one float, or {sid: float} (sessions not
        in it: 1.0).  An empty dict makes no library call."""
        if not isinstance(chunks, dict):
            raise ValueError("StreamPool.step: chunks must be a dict {session id: tensor}, got %s" % type(chunks).__name__)
        n = None
        for sid, t in chunks.items():
            self._rows_of(sid)
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != self.rows:
                raise ValueError("StreamPool.step: session %r needs a tensor [%d, L*1024], got %s" % (
                    sid, self.rows, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
            if t.shape[1] % _spec.HOP or t.shape[1] == 0:
                raise ValueError("StreamPool.step: session %r holds %d samples per row, need whole hops of 1024" % (sid, t.shape[1]))
            if n is not None and t.shape[1] != n:
                raise ValueError("StreamPool.step: session %r holds %d samples per row, the others %d (one L per step)" % (sid, t.shape[1], n))
            n = t.shape[1]
            if sid in self._rate:
                raise ValueError("StreamPool.step: session %r has a sample rate of its own (%d Hz): its audio does not come in whole hops, "
                                 "use feed()" % (sid, self.rates[self._rate[sid]]))
        per_row = isinstance(mix, dict)
        if per_row:
            for sid, v in mix.items():
                self._rows_of(sid)
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError("StreamPool.step: mix of session %r must be a float, got %s" % (sid, type(v).__name__))
        elif mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("StreamPool.step: mix must be None, a float or a dict {session id: float}, got %s" % type(mix).__name__)
        if not chunks:
            return {}
        st = self._stream()
        C = self.slots * self.rows
        wave = torch.zeros((C, n), dtype=torch.float32, device=st.device)
        active = [False] * C
        mix_rows = [1.0] * C
        for sid, t in chunks.items():
            rows = self._rows_of(sid)
            wave[rows.start:rows.stop] = t.detach().to(device=st.device, dtype=torch.float32)
            for r in rows:
                active[r] = True
                if per_row:
                    mix_rows[r] = float(mix.get(sid, 1.0))
        m = torch.tensor(mix_rows, dtype=torch.float32) if per_row else (1.0 if mix is None else float(mix))
        out = st.process_rows(wave, active, m)
        res = {}
        for sid, t in chunks.items():
            rows = self._rows_of(sid)
            o = out[rows.start:rows.stop]
            res[sid] = o.clone() if t.is_cuda else o.cpu()
        return res

    def export(self, sid):
        """-> the session's carry, one blob (CPU tensor) per row, for adopt() of this or another pool of the same model."""
        rows = self._rows_of(sid)
        if sid in self._rate:
            raise ValueError("StreamPool.export: session %r has a sample rate of its own (%d Hz); the resamplers' carries do not move "
                             "with a session" % (sid, self.rates[self._rate[sid]]))
        st = self._stream()
        return [st.get_row(r) for r in rows]

    def drain(self, sid, mix=None):
        """The session's audio ends: -> the tail it is still owed, [rows_per_session, n] on the pool's device, at the session's rate.  In
        order: the inbound resampler's rows are flushed (the future counting as zeros); what waits is padded with zeros to a whole hop;
        one more hop of zeros follows for the stream's one-hop delay; those hops run with every other session held; the outbound
        resampler converts them and is flushed.  Afterwards the session's rows of the stream and of both banks are reset: it stays open
        and its next feed() begins a new piece of audio.  A session without a rate skips the resampler steps: it gets the padded hops
        and the extra one as the stream gives them.
        LENGTH: a session that fed n samples at its rate r since it was opened (or drained) has received, feed() results and this tail
        together, resample_len(m, 44100, r) samples with m = resample_len(n, r, 44100) rounded up to whole hops of 1024.
        mix: None or one float, as in feed()."""
        rows = self._rows_of(sid)
        if mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("StreamPool.drain: mix must be None or a float, got %s" % type(mix).__name__)
        st = self._stream()
        rated = sid in self._rate
        lst = list(rows)
        if rated:
            out, got = self._bank_in.flush_rows(lst)
            x = out[rows.start:rows.stop, :got[rows.start]]
        else:
            x = torch.empty((self.rows, 0), dtype=torch.float32, device=st.device)
        hop = _spec.HOP
        pad = -(self.pending(sid) + x.shape[1]) % hop
        x = torch.cat((x, torch.zeros((self.rows, pad + hop), dtype=torch.float32, device=st.device)), 1)
        tail = self._feed_hops({sid: x}, mix)[sid]
        if rated:
            a = self._bank_call(self._bank_out, {sid: self._undelayed(sid, tail)})[sid]
            out, got = self._bank_out.flush_rows(lst)
            tail = torch.cat((a, out[rows.start:rows.stop, :got[rows.start]]), 1)
            self._skip[sid] = hop
        st.reset_rows(lst)
        self._pend.pop(sid, None)
        return tail

    def adopt(self, blobs):
        """A session exported elsewhere continues here, bit for bit -> its new id (a session without a sample rate of its own)."""
        blobs = list(blobs)
        nf = 2 * _spec.N_FFT + 8 * len(self.model.band_widths) * band_features
        if len(blobs) != self.rows or not all(isinstance(b, torch.Tensor) and b.dim() == 1 and b.numel() == nf for b in blobs):
            raise ValueError("StreamPool.adopt: need %d blobs of %d floats each" % (self.rows, nf))
        if not self._free:
            raise ValueError("StreamPool: all %d slots are in use" % self.slots)
        st = self._stream()
        sid = self.open()
        for r, b in zip(self._rows_of(sid), blobs):
            st.set_row(r, b)
        return sid


class NativeStreamPool:
    """StreamPool's sessions at the model's rate as an object of the LIBRARY (bsrnn_pool_*, include/bsrnn_hip.h): the slots, the samples
    that wait for a whole hop (a device-resident FIFO per row) and the packing of every session's audio around the one
    bsrnn_stream_process_hops of a tick all live behind ONE library call per feed, which takes a pointer per session.  Nothing is
    copied on the host: a CUDA chunk goes by its pointer and row stride (views are fine; float32 with unit inner stride), and the
    results are views of one tensor allocated per feed.  A dict of CPU tensors takes the library's host form (bsrnn_pool_feed_host).
    Same numbers as StreamPool: both make the same hops calls on the same samples (a feed of more than max_hops hops runs in rounds of
    max_hops, where StreamPool's rounds are 255 hops long).  The pool is created at the first call that needs the device; shape and
    type errors are raised before that.  Sessions with a sample rate of their own: the subclass NativeRatePool (or StreamPool(rates=...))."""

    MODEL_RATE = 44100

    def __init__(self, model, slots, rows_per_session=1, device=None, max_hops=8):
        for name, v in (("slots", slots), ("rows_per_session", rows_per_session), ("max_hops", max_hops)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("NativeStreamPool: %s must be a positive int, got %r" % (name, v))
        if slots * rows_per_session > _native.STREAM_ROWS_MAX:
            raise ValueError("NativeStreamPool: %d slots x %d rows is more than the %d rows a rows call takes" % (
                slots, rows_per_session, _native.STREAM_ROWS_MAX))
        if max_hops > _native.STREAM_HOPS_MAX:
            raise ValueError("NativeStreamPool: max_hops = %d, a hops call takes at most %d" % (max_hops, _native.STREAM_HOPS_MAX))
        self.model, self.slots, self.rows, self.max_hops = model, int(slots), int(rows_per_session), int(max_hops)
        self._device = device
        self.device = None                  # set with the pool
        self._h = None
        self._slot = {}                     # session id -> slot
        self._free = list(range(self.slots))
        self._next = 0
        self._steps = 0

    def __del__(self):
        try:
            if self._h is not None:
                _lib.bsrnn_pool_destroy(self._h)
        except Exception:
            pass

    def _pool(self):
        if self._h is None:
            self.device = torch.device("cuda", torch.cuda.current_device()) if self._device is None else torch.device(self._device)
            with torch.cuda.device(self.device):
                ctx = self.model._context(self.device)
                h = ctypes.c_void_p()
                self._create(ctx, h)
                self._h = h
                # the sessions opened so far: the library hands out the lowest free slot, as open() did
                used = set(self._slot.values())
                got = ctypes.c_int32()
                for k in range(max(used) + 1 if used else 0):
                    self._open_slot(h, k, got)
                    assert got.value == k
                for k in range(max(used) + 1 if used else 0):
                    if k not in used:
                        _check(_lib.bsrnn_pool_close(h, k))
        return self._h

    def _create(self, ctx, h):
        _check(_lib.bsrnn_pool_create(ctx, self.slots, self.rows, self.max_hops, ctypes.byref(h)))

    def _open_slot(self, h, slot, got):
        _check(_lib.bsrnn_pool_open(h, ctypes.byref(got)))

    def _n_out(self, sid, n):
        """Samples per row the session's next feed of n gives."""
        return (self.pending(sid) + n) // _spec.HOP * _spec.HOP

    def _look_at_weights(self):
        # the same look at the model's parameters as StreamingSeparator.step() takes (see there), once per call
        if self._steps % 32 == 0 or self.model._weights_touched(self._steps):
            self.model._plist = None
            with torch.cuda.device(self.device):
                self.model._context(self.device)
        self._steps += 1

    def _rows_of(self, sid):
        slot = self._slot[sid]              # KeyError: no such session
        return range(slot * self.rows, (slot + 1) * self.rows)

    def sessions(self):
        return list(self._slot)

    def open(self, sample_rate=None):
        """-> a new session's id; its rows start from silence and nothing waits.  ValueError when every slot is taken, and for a
        sample_rate other than None or the model's 44100."""
        if sample_rate is not None and sample_rate != self.MODEL_RATE:
            raise ValueError("NativeStreamPool.open: sample_rate %r: the native pool serves sessions at the model's %d Hz; sessions with a "
                             "rate of their own are StreamPool(rates=...)'s" % (sample_rate, self.MODEL_RATE))
        if not self._free:
            raise ValueError("NativeStreamPool: all %d slots are in use" % self.slots)
        slot = self._free.pop(0)
        if self._h is not None:
            got = ctypes.c_int32()
            with torch.cuda.device(self.device):
                _check(_lib.bsrnn_pool_open(self._h, ctypes.byref(got)))
            assert got.value == slot
        sid, self._next = self._next, self._next + 1
        self._slot[sid] = slot
        return sid

    def close(self, sid):
        """The session leaves; samples of it that waited are dropped."""
        slot = self._slot.pop(sid)
        self._free.append(slot)
        self._free.sort()
        if self._h is not None:
            _check(_lib.bsrnn_pool_close(self._h, slot))

    def pending(self, sid):
        """Samples per row of the session that wait for its next feed() (fewer than one hop)."""
        slot = self._slot[sid]
        return 0 if self._h is None else int(_lib.bsrnn_pool_pending(self._h, slot))

    def _check_mix(self, mix, who):
        if isinstance(mix, dict):
            for sid, v in mix.items():
                self._rows_of(sid)
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError("NativeStreamPool.%s: mix of session %r must be a float, got %s" % (who, sid, type(v).__name__))
        elif mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("NativeStreamPool.%s: mix must be None, a float or a dict {session id: float}, got %s" % (who, type(mix).__name__))

    def feed(self, chunks, mix=None):
        """chunks {sid: tensor [rows_per_session, n]}, ANY n >= 0 and another one per session, all CUDA tensors on the pool's device or all
        CPU tensors -> {sid: tensor [rows_per_session, h*1024] on the same device}: every session advances by the h = (pending + n) //
        1024 hops it has in hand, in ONE library call (bsrnn_pool_feed / _feed_host); the remainder waits on the device.  Sessions not
        named are held.  mix: None (1.0), one float, or {sid: float} (sessions not in it: 1.0).  The chunks must be float32 with unit
        inner stride (a row stride of any size: column slices and views with a storage offset go by pointer, uncopied); the results
        are views of one tensor made by this call."""
        if not isinstance(chunks, dict):
            raise ValueError("NativeStreamPool.feed: chunks must be a dict {session id: tensor}, got %s" % type(chunks).__name__)
        on_cuda = None
        for sid, t in chunks.items():
            self._rows_of(sid)
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != self.rows:
                raise ValueError("NativeStreamPool.feed: session %r needs a tensor [%d, n], got %s" % (
                    sid, self.rows, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
            if t.dtype != torch.float32:
                raise ValueError("NativeStreamPool.feed: session %r needs float32 samples, got %s (the chunk goes by pointer)" % (sid, t.dtype))
            n = t.shape[1]
            if n and (t.stride(1) != 1 or (self.rows > 1 and t.stride(0) < n)):
                raise ValueError("NativeStreamPool.feed: session %r: strides %r; the chunk goes by pointer and row stride, so samples of a row "
                                 "must be adjacent and rows must not overlap" % (sid, tuple(t.stride())))
            if on_cuda is not None and t.is_cuda != on_cuda:
                raise ValueError("NativeStreamPool.feed: CUDA and CPU chunks in one call; a feed takes one kind")
            on_cuda = t.is_cuda
        self._check_mix(mix, "feed")
        if not chunks:
            return {}
        h = self._pool()
        for sid, t in chunks.items():
            if t.is_cuda and t.device != self.device:
                raise ValueError("NativeStreamPool.feed: session %r brings a chunk on %s, the pool lives on %s" % (sid, t.device, self.device))
        self._look_at_weights()
        n_s = len(chunks)
        sids = list(chunks)
        n_out = [self._n_out(sid, chunks[sid].shape[1]) for sid in sids]
        block = torch.empty((self.rows * sum(n_out),), dtype=torch.float32, device=self.device if on_cuda else "cpu")
        res, at = {}, 0
        for sid, m in zip(sids, n_out):
            res[sid] = block[at:at + self.rows * m].view(self.rows, m)
            at += self.rows * m
        keep = [chunks[sid].detach() for sid in sids]
        slots = (ctypes.c_int32 * n_s)(*[self._slot[sid] for sid in sids])
        in_p = (ctypes.c_void_p * n_s)(*[t.data_ptr() if t.shape[1] else None for t in keep])
        in_s = (ctypes.c_int64 * n_s)(*[max(t.stride(0), t.shape[1]) if self.rows > 1 else t.shape[1] for t in keep])
        n_in = (ctypes.c_int64 * n_s)(*[t.shape[1] for t in keep])
        out_p = (ctypes.c_void_p * n_s)(*[res[sid].data_ptr() if m else None for sid, m in zip(sids, n_out)])
        out_s = (ctypes.c_int64 * n_s)(*n_out)
        got = (ctypes.c_int64 * n_s)()
        if isinstance(mix, dict):
            mix_p, mix_v = (ctypes.c_float * n_s)(*[float(mix.get(sid, 1.0)) for sid in sids]), 1.0
        else:
            mix_p, mix_v = None, 1.0 if mix is None else float(mix)
        with torch.cuda.device(self.device):
            if on_cuda:
                _check(_lib.bsrnn_pool_feed(h, n_s, slots, in_p, in_s, n_in, out_p, out_s, got, mix_p, mix_v, _stream_ptr(self.device)))
            else:
                _check(_lib.bsrnn_pool_feed_host(h, n_s, slots, in_p, in_s, n_in, out_p, out_s, got, mix_p, mix_v))
        assert list(got) == n_out
        return res

    def step(self, chunks, mix=None):
        """A feed whose chunks are whole hops, one L for all: chunks {sid: tensor [rows_per_session, L*1024]} -> {sid: tensor of the same
        shape}, delayed by one hop.  An empty dict makes no library call."""
        if not isinstance(chunks, dict):
            raise ValueError("NativeStreamPool.step: chunks must be a dict {session id: tensor}, got %s" % type(chunks).__name__)
        n = None
        for sid, t in chunks.items():
            self._rows_of(sid)
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != self.rows:
                raise ValueError("NativeStreamPool.step: session %r needs a tensor [%d, L*1024], got %s" % (
                    sid, self.rows, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
            if t.shape[1] % _spec.HOP or t.shape[1] == 0:
                raise ValueError("NativeStreamPool.step: session %r holds %d samples per row, need whole hops of 1024" % (sid, t.shape[1]))
            if n is not None and t.shape[1] != n:
                raise ValueError("NativeStreamPool.step: session %r holds %d samples per row, the others %d (one L per step)" % (sid, t.shape[1], n))
            n = t.shape[1]
        self._check_mix(mix, "step")
        return self.feed(chunks, mix)

    def _row_floats(self):
        return 2 * _spec.N_FFT + 8 * len(self.model.band_widths) * band_features

    def export(self, sid):
        """-> (blobs, pending): the session's carry, one blob (CPU tensor) per row as StreamPool.export gives them, and the samples that
        wait, a CPU tensor [rows_per_session, pending(sid)] - everything adopt() of this or another pool of the same model needs to
        continue the session bit for bit, in the middle of a hop too."""
        rows = self._rows_of(sid)
        h = self._pool()
        st = _lib.bsrnn_pool_stream(h)
        blobs = []
        for r in rows:
            b = np.empty(self._row_floats(), np.float32)
            _check(_lib.bsrnn_stream_get_row(st, r, b.ctypes.data_as(ctypes.c_void_p)))
            blobs.append(torch.from_numpy(b))
        fifo = np.empty((self.rows, _spec.HOP), np.float32)
        n = ctypes.c_int32()
        _check(_lib.bsrnn_pool_get_pending(h, self._slot[sid], fifo.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n)))
        return blobs, torch.from_numpy(fifo[:, :n.value].copy())

    def adopt(self, blobs, pending=None):
        """A session exported elsewhere - adopt(*other.export(sid)), or the blobs of StreamPool.export alone - continues here, bit for
        bit -> its new id."""
        blobs = list(blobs)
        nf = self._row_floats()
        if len(blobs) != self.rows or not all(isinstance(b, torch.Tensor) and b.dim() == 1 and b.numel() == nf for b in blobs):
            raise ValueError("NativeStreamPool.adopt: need %d blobs of %d floats each" % (self.rows, nf))
        if pending is not None and (not isinstance(pending, torch.Tensor) or pending.dim() != 2 or pending.shape[0] != self.rows or
                                    pending.shape[1] >= _spec.HOP):
            raise ValueError("NativeStreamPool.adopt: pending must be a tensor [%d, n] with n < %d, got %s" % (
                self.rows, _spec.HOP, tuple(pending.shape) if isinstance(pending, torch.Tensor) else type(pending).__name__))
        if not self._free:
            raise ValueError("NativeStreamPool: all %d slots are in use" % self.slots)
        h = self._pool()
        sid = self.open()
        st = _lib.bsrnn_pool_stream(h)
        for r, b in zip(self._rows_of(sid), blobs):
            a = np.ascontiguousarray(b.detach().to("cpu", torch.float32).numpy())
            _check(_lib.bsrnn_stream_set_row(st, r, a.ctypes.data_as(ctypes.c_void_p)))
        if pending is not None and pending.shape[1]:
            fifo = np.zeros((self.rows, _spec.HOP), np.float32)
            fifo[:, :pending.shape[1]] = pending.detach().to("cpu", torch.float32).numpy()
            _check(_lib.bsrnn_pool_set_pending(h, self._slot[sid], fifo.ctypes.data_as(ctypes.c_void_p), int(pending.shape[1])))
        return sid


class NativeRatePool(NativeStreamPool):
    """A NativeStreamPool whose sessions may give and get audio at a sample rate of their own, one of `rates` (at most 16, checked as
    StreamPool(rates=...) checks them): the library's bsrnn_pool_create_rates / _open_rate / _drain.  A tick is still ONE library call:
    what all such sessions bring goes to the model's 44.1 kHz in one inbound launch of a resampler bank (reading at the sessions' own
    pointers), everybody's hops run as before, and one outbound launch converts the result to the sessions' rates at the pointers of
    their outputs; the stream's one-hop delay is taken out of such a session's audio and drain() ends it.  Same numbers as
    StreamPool(rates=...), bit for bit, where the rounds coincide (a feed of at most max_hops hops).  max_block: the most samples per
    row, at its own rate, a session with a rate brings in one feed; the pool's staging is sized by it at creation.  Sessions with a
    rate take CUDA chunks only, and stay in their pool (export refuses them)."""

    def __init__(self, model, slots, rows_per_session=1, device=None, max_hops=8, rates=(48000,), max_block=48000):
        rates = StreamPool._checked_rates(rates)
        if rates is None:
            raise ValueError("NativeRatePool: rates must be a tuple of sample rates, got None (a pool without is NativeStreamPool)")
        if isinstance(max_block, bool) or not isinstance(max_block, (int, np.integer)) or not 1 <= max_block <= 1 << 24:
            raise ValueError("NativeRatePool: max_block must be an int in [1, 2^24], got %r" % (max_block,))
        super().__init__(model, slots, rows_per_session, device, max_hops)
        self.rates, self.max_block = rates, int(max_block)
        self._rate = {}                     # session id -> index into rates, for the sessions that have one

    def _create(self, ctx, h):
        rates = (ctypes.c_int32 * len(self.rates))(*self.rates)
        _check(_lib.bsrnn_pool_create_rates(ctx, self.slots, self.rows, self.max_hops, rates, len(self.rates), self.max_block, ctypes.byref(h)))

    def _open_slot(self, h, slot, got):
        rate = self.MODEL_RATE
        for sid, k in self._rate.items():
            if self._slot[sid] == slot:
                rate = self.rates[k]
        _check(_lib.bsrnn_pool_open_rate(h, rate, ctypes.byref(got)))

    def _n_out(self, sid, n):
        return int(_lib.bsrnn_pool_ready(self._h, self._slot[sid], n))

    def open(self, sample_rate=None):
        """-> a new session's id; its rows start from silence and nothing waits.  sample_rate: None or the model's 44100 for a session
        at the model's rate, else one of the pool's `rates`.  ValueError when every slot is taken or the rate is not one of them."""
        k = None
        if sample_rate is not None and sample_rate != self.MODEL_RATE:
            if sample_rate not in self.rates:
                raise ValueError("NativeRatePool.open: sample_rate %r is not one of the pool's rates %r" % (sample_rate, self.rates))
            k = self.rates.index(sample_rate)
        if not self._free:
            raise ValueError("NativeRatePool: all %d slots are in use" % self.slots)
        slot = self._free.pop(0)
        sid, self._next = self._next, self._next + 1
        self._slot[sid] = slot
        if k is not None:
            self._rate[sid] = k
        if self._h is not None:
            got = ctypes.c_int32()
            with torch.cuda.device(self.device):
                self._open_slot(self._h, slot, got)
            assert got.value == slot
        return sid

    def close(self, sid):
        """The session leaves; samples of it that waited are dropped and its rows of the resampler banks start afresh."""
        super().close(sid)
        self._rate.pop(sid, None)

    def rate_of(self, sid):
        """The session's sample rate (44100 for one opened without)."""
        self._rows_of(sid)
        return self.rates[self._rate[sid]] if sid in self._rate else self.MODEL_RATE

    def feed(self, chunks, mix=None):
        """NativeStreamPool.feed; a session opened with a sample rate gives its chunk AT THAT RATE (a CUDA tensor of at most max_block
        samples per row) and gets back, at that rate, the output samples that have become determined - bsrnn_pool_ready's count, which
        varies from tick to tick.  pending() stays a count at the model's rate."""
        if isinstance(chunks, dict):
            for sid, t in chunks.items():
                if sid in self._rate and isinstance(t, torch.Tensor) and t.dim() == 2:
                    if t.shape[1] > self.max_block:
                        raise ValueError("NativeRatePool.feed: session %r brings %d samples per row, the pool was created for max_block = %d"
                                         % (sid, t.shape[1], self.max_block))
                    if not t.is_cuda:
                        raise ValueError("NativeRatePool.feed: session %r has a sample rate of its own (%d Hz) and brings a CPU chunk; the "
                                         "host form serves sessions at the model's rate" % (sid, self.rates[self._rate[sid]]))
        return super().feed(chunks, mix)

    def step(self, chunks, mix=None):
        """NativeStreamPool.step, for sessions at the model's rate."""
        if isinstance(chunks, dict):
            for sid in chunks:
                if sid in self._rate:
                    raise ValueError("NativeRatePool.step: session %r has a sample rate of its own (%d Hz): its audio does not come in whole "
                                     "hops, use feed()" % (sid, self.rates[self._rate[sid]]))
        return super().step(chunks, mix)

    def export(self, sid):
        """NativeStreamPool.export, for a session at the model's rate."""
        self._rows_of(sid)
        if sid in self._rate:
            raise ValueError("NativeRatePool.export: session %r has a sample rate of its own (%d Hz); the resamplers' carries do not move "
                             "with a session" % (sid, self.rates[self._rate[sid]]))
        return super().export(sid)

    def drain(self, sid, mix=None):
        """The session's audio ends: -> the tail it is still owed, [rows_per_session, n] on the pool's device, at the session's rate -
        StreamPool.drain's steps and its LENGTH rule, in one library call (bsrnn_pool_drain).  The session stays open and its next feed()
        begins a new piece of audio.  mix: None or one float."""
        slot = self._slot[sid]
        if mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("NativeRatePool.drain: mix must be None or a float, got %s" % type(mix).__name__)
        h = self._pool()
        self._look_at_weights()
        n = int(_lib.bsrnn_pool_drain_len(h, slot))
        out = torch.empty((self.rows, n), dtype=torch.float32, device=self.device)
        got = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_pool_drain(h, slot, out.data_ptr() if n else None, n, ctypes.byref(got), 1.0 if mix is None else float(mix),
                                         _stream_ptr(self.device)))
        assert got.value == n
        return out
