"""Streaming sample-rate conversion on the device: Resampler (bsrnn_resampler_*), one rate pair and one clock for all rows, and
ResamplerBank (bsrnn_resampler_bank_*), a pair, a count and a stream position per row.  The one-shot form is BSRNN.resample, which
is why resample_len, the count all of them go by, stays beside the model.  `from speechseparation_amd.bsrnn import Resampler,
ResamplerBank` gives the same classes."""
import ctypes
import math

import numpy as np
import torch

from . import _native
from .bsrnn import BSRNN, _check, _lib, _ptr, _stream_ptr, resample_len


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
