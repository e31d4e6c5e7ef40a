"""Host-side mirror of the reference's `bsrnn.py` operator interface, running on libbsrnn_hip.

Same surface as the reference model class (bsrnn.py:328-510):
    BSRNN()                                   no constructor arguments (band table optional here)
    .to(device) / .eval() / .state_dict() / .load_state_dict(sd)   -- identical key names and
                                              shapes (288 tensors)
    .forward(x [C,2050,T]) -> [C,2050,T]      bsrnn.py:385
    .forward_recurrent(x [C,2050], state [4,2,C*K,64]) -> (y, new_state)   bsrnn.py:445
    generate_bandsplits(), band_features, merge_channels module globals    bsrnn.py:247, :60-61
plus the fused device-side sandwich of the callers (`separate`, `stft`, `istft`); the chunked
streaming form is in streaming.py, resample.py and pool.py.  The torch modules below are *parameter containers only* (they give the
state_dict its names, shapes and default initialisation); their own forward() is never
called -- all arithmetic happens in hand-written HIP kernels behind the C ABI, and without
the built library this module cannot be imported (no CPU fallback).
"""
import ctypes

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


def resample_len(n_in, rate_in, rate_out):
    """Samples bsrnn_resample gives for n_in: ceil(n_in * up / down).  ValueError for what the library refuses (a rate < 1, a reduced
    max(up, down) beyond 1024, n_in < 1)."""
    n = _lib.bsrnn_resample_len(int(n_in), int(rate_in), int(rate_out))
    if n < 0:
        raise ValueError("resample: cannot convert %s samples from %s to %s Hz (rates >= 1, reduced max(up, down) <= 1024, n >= 1)" % (
            n_in, rate_in, rate_out))
    return n


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


# The streaming classes live in modules of their own (streaming.py, resample.py, pool.py), which import this one and which this one
# does not import; `from speechseparation_amd.bsrnn import StreamPool` and the like stay valid and give the same objects.
_MOVED = {"StreamingSeparator": "streaming",
          "Resampler": "resample", "ResamplerBank": "resample",
          "StreamPool": "pool", "NativeStreamPool": "pool", "NativeRatePool": "pool"}


def __getattr__(name):
    if name in _MOVED:
        import importlib
        return getattr(importlib.import_module("." + _MOVED[name], __package__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
