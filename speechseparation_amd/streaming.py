"""The chunked streaming form of the model: StreamingSeparator, one device-resident stream of C rows (bsrnn_stream_*), and the two
things the session pools of pool.py share with it - the look a running stream takes at the model's weights, and the size of a row's
carry.  `from speechseparation_amd.bsrnn import StreamingSeparator` gives the same class."""
import ctypes

import numpy as np
import torch

from . import _native
from . import spec as _spec
from .bsrnn import _check, _lib, _ptr, _stream_ptr, band_features


def look_at_weights(owner):
    """Once per streaming call of `owner` (a StreamingSeparator or a native pool: .model, .device, ._steps)."""
    # The reference's forward_recurrent always sees the current parameters (bsrnn.py:445).  Here the weights live packed on the
    # device, so a running stream looks at the model every step, cheaply: a rotating eighth of the parameters' version counters
    # and storage pointers per step (an optimizer step or load_state_dict is seen at the next chunk, an in-place edit or
    # rebinding of a single tensor within 8 chunks), and the whole module tree again every 32nd step (a parameter OBJECT
    # swapped into a submodule).  model.refresh_weights() forces it at once.
    if owner._steps % 32 == 0 or owner.model._weights_touched(owner._steps):
        owner.model._plist = None           # (re-read the parameter objects and their storage pointers)
        with torch.cuda.device(owner.device):
            owner.model._context(owner.device)
    owner._steps += 1


def row_floats(model):
    """Floats of one row's carry as get_row / set_row move it: buf[2048], prev[2048], state[4][2][K][64]."""
    return 2 * _spec.N_FFT + 8 * len(model.band_widths) * band_features


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
        look_at_weights(self)
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
        look_at_weights(self)
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
    def _check_row(self, row, what):
        if isinstance(row, bool) or not isinstance(row, (int, np.integer)):
            raise ValueError("%s: row must be an int, got %s" % (what, type(row).__name__))
        if not 0 <= row < self.C:
            raise ValueError("%s: row %d is outside [0, %d)" % (what, row, self.C))
        return int(row)

    def row_floats(self):
        """Floats of one row's carry as get_row / set_row move it: buf[2048], prev[2048], state[4][2][K][64]."""
        return row_floats(self.model)

    def _hops_of(self, wave, who):
        """The wave check of the rows calls -> L, its whole hops per row."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("%s: expected wave [%d, L*1024], got %s" % (
                who, self.C, tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__))
        if wave.shape[1] % _spec.HOP:
            raise ValueError("%s: wave must hold whole hops of 1024 samples, got %d samples per row" % (who, wave.shape[1]))
        return wave.shape[1] // _spec.HOP

    def _mix_of(self, mix, who):
        """The mix check of the rows calls -> (the [C] tensor or None, the one value)."""
        if isinstance(mix, torch.Tensor):
            if tuple(mix.shape) != (self.C,):
                raise ValueError("%s: mix must be a float or a tensor [%d], got %s" % (who, self.C, tuple(mix.shape)))
            return mix, 1.0
        if isinstance(mix, bool) or not isinstance(mix, (int, float, np.floating, np.integer)):
            raise ValueError("%s: mix must be a float or a tensor [%d], got %s" % (who, self.C, type(mix).__name__))
        return None, mix

    def _rows_call(self, call, wave, L, per_row, mix_rows, mix):
        """The tail of the rows calls, behind their checks: `call` is the library's function, per_row its array of one entry per row."""
        if L == 0:
            return torch.empty((self.C, 0), dtype=torch.float32, device=wave.device)
        look_at_weights(self)
        x = wave.detach().to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty_like(x)
        if mix_rows is not None:
            mix_rows = mix_rows.detach().to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            _check(call(self._h, _ptr(x), _ptr(out), L, per_row, _ptr(mix_rows) if mix_rows is not None else None, float(mix),
                        _stream_ptr(self.device)))
        return out if wave.is_cuda else out.cpu()

    def process_rows(self, wave, active=None, mix=1.0):
        """wave [C, L*1024] float32 (cuda or cpu), whole hops -> [C, L*1024] on the same device (bsrnn_stream_process_rows): rows with a
        true entry in `active` (a sequence or tensor of C flags; None: every row) take the L hops exactly as process() would give them,
        the others are HELD - their carry stays bit for bit, their output rows are zeros and their input rows are never read.  `mix` is
        one wet / dry value or a [C] tensor of one per row.  Takes no part in process()'s carrying of partial hops."""
        L = self._hops_of(wave, "process_rows")
        act = None
        if active is not None:
            try:
                flags = [bool(a) for a in (active.tolist() if isinstance(active, (torch.Tensor, np.ndarray)) else active)]
            except TypeError:
                raise ValueError("process_rows: active must be a sequence of %d flags, got %s" % (self.C, type(active).__name__)) from None
            if len(flags) != self.C:
                raise ValueError("process_rows: %d flags for %d rows" % (len(flags), self.C))
            act = (ctypes.c_uint8 * self.C)(*flags)
        mix_rows, mix = self._mix_of(mix, "process_rows")
        return self._rows_call(_lib.bsrnn_stream_process_rows, wave, L, act, mix_rows, mix)

    def process_hops(self, wave, hops, mix=1.0):
        """wave [C, L*1024] float32 (cuda or cpu), whole hops, and hops, a sequence or tensor of C ints in [0, L] -> [C, L*1024] on the same
        device, from one library call (bsrnn_stream_process_hops): row r takes its first hops[r] hops exactly as that many step() calls
        would give them, its output row is zeros behind them, its input row is never read behind them, and its carry is the one after
        hops[r] hops; a row at 0 is held as by process_rows.  At most 255 hops per call.  `mix` is one wet / dry value or a [C] tensor
        of one per row.  Takes no part in process()'s carrying of partial hops."""
        L = self._hops_of(wave, "process_hops")
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
        mix_rows, mix = self._mix_of(mix, "process_hops")
        cnt = (ctypes.c_int32 * self.C)(*[int(h) for h in counts])
        return self._rows_call(_lib.bsrnn_stream_process_hops, wave, L, cnt, mix_rows, mix)

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
