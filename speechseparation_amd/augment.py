"""The reference's two training augmentations on the device: room impulse responses (m_dataset.py:92-114) and the re-mix of
MixDataSet (:141-180).

The reference convolves a clip with a whole room impulse response - tens of thousands of taps - through
torch.nn.functional.conv1d(padding='same').  `FirBank` computes the same function with the library's partitioned FFT convolution
(include/bsrnn_hip.h, bsrnn_convolve_ragged): rows of different lengths, each under its own filter, in one call.  `rir_draw` makes the
reference's random decisions for a clip, `reverb_pairs` applies them to the clips of an optimizer step, `remix` is MixDataSet's arithmetic.
`FirStream` is the hop-by-hop form of `FirBank.convolve` for live streams (bsrnn_fir_stream_*).
`SourceShelf`, `remix_draw` and `remix_many` are MixDataSet as a loader: sources held on the device, the reference's draws on the host,
and the mixtures and targets of an optimizer step written by one bsrnn_remix_ragged into the buffers train.train_loss_ragged takes.
"""
import ctypes
import random
from typing import NamedTuple

import numpy as np
import torch

from . import _native
from .bsrnn import BSRNN, _ptr, _stream_ptr

_lib = _native.lib
_check = _native.check
MAX_TAPS = 262144                           # CONV_MAX_TAPS of csrc/convolve_host.h


class FirBank:
    """A set of FIR filters on the model's device (bsrnn_fir_bank_*): `filters` is a list of 1-D float32 arrays or tensors of 1 ... 262144
    taps.  Their partition spectra are built once, here.  `convolve` applies them as torch.nn.functional.conv1d(x, h, padding='same') does."""

    def __init__(self, model, filters):
        filters = list(filters)
        if not filters:
            raise ValueError("FirBank: need at least one filter")
        taps = []
        for i, h in enumerate(filters):
            a = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
            if a.ndim != 1 or a.dtype != np.float32 or not 1 <= a.shape[0] <= MAX_TAPS:
                raise ValueError("FirBank: filter %d must be a 1-D float32 array of 1 ... %d taps, got %s %s" % (i, MAX_TAPS, a.shape, a.dtype))
            taps.append(np.ascontiguousarray(a))
        self.model = model
        self.device = torch.device("cuda", model._ctx_device if model._ctx_device is not None else torch.cuda.current_device())
        n = len(taps)
        ptrs = (ctypes.c_void_p * n)(*[t.ctypes.data for t in taps])
        counts = (ctypes.c_int32 * n)(*[t.shape[0] for t in taps])
        with torch.cuda.device(self.device):
            ctx = model._context(self.device)
            h = ctypes.c_void_p()
            _check(_lib.bsrnn_fir_bank_create(ctx, n, ptrs, counts, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        try:
            _lib.bsrnn_fir_bank_destroy(self._h)
        except Exception:
            pass

    def __len__(self):
        return int(_lib.bsrnn_fir_bank_count(self._h))

    def taps(self, i):
        k = int(_lib.bsrnn_fir_bank_taps(self._h, int(i)))
        if k < 0:
            raise IndexError("FirBank.taps: filter %r of %d" % (i, len(self)))
        return k

    def convolve(self, wave, lengths=None, filters=None, out=None):
        """wave [R, n_max] float32 on the bank's device -> out [R, n_max]: out[r, :lengths[r]] = conv1d(wave[r, :lengths[r]], filter
        filters[r], padding='same'); a filter of -1 copies the row, bit for bit.  lengths defaults to n_max for every row, filters to
        filter 0.  What lies behind a row's length is not read, and in a given `out` not written (a new `out` holds zeros there).  Views
        with a row stride (buf[:, a:b], a channel slice) go by pointer, uncopied; `out` must not overlap the input."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] < 1 or wave.shape[1] < 1:
            raise ValueError("FirBank.convolve: expected wave [R, n_max] with n_max >= 1, got %s" % (
                tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__,))
        if wave.dtype != torch.float32:
            raise ValueError("FirBank.convolve: expected a float32 tensor, got %s" % wave.dtype)
        if not wave.is_cuda:
            raise _native.NativeError("FirBank.convolve: the waveform must be on a HIP device")
        if wave.device != self.device:
            raise ValueError("FirBank.convolve: the waveform is on %s, the bank on %s" % (wave.device, self.device))
        R, n_max = wave.shape
        lens = [n_max] * R if lengths is None else [int(n) for n in lengths]
        filt = [0] * R if filters is None else [int(f) for f in filters]
        if len(lens) != R or len(filt) != R:
            raise ValueError("FirBank.convolve: %d lengths and %d filters for %d rows" % (len(lens), len(filt), R))
        for r in range(R):
            if not 1 <= lens[r] <= n_max:
                raise ValueError("FirBank.convolve: row %d has length %d, need 1 <= length <= %d" % (r, lens[r], n_max))
            if not -1 <= filt[r] < len(self):
                raise ValueError("FirBank.convolve: row %d names filter %d of %d" % (r, filt[r], len(self)))
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != wave.device
                                or tuple(out.shape) != (R, n_max) or (out.stride(1) != 1 and n_max > 1) or (R > 1 and out.stride(0) < n_max)):
            raise ValueError("FirBank.convolve: out must be a float32 tensor %s with contiguous rows that do not overlap on %s" % ((R, n_max), wave.device))
        w, w_stride = BSRNN._rows_view(wave.detach())
        with torch.cuda.device(self.device):
            if out is None:
                out = torch.zeros((R, n_max), device=self.device, dtype=torch.float32)
            o_stride = out.stride(0) if R > 1 else n_max
            _check(_lib.bsrnn_convolve_ragged(self._h, _ptr(w), w_stride, (ctypes.c_int64 * R)(*lens), (ctypes.c_int32 * R)(*filt), _ptr(out),
                                              o_stride, R, _stream_ptr(self.device)))
        return out


class FirStream:
    """The streaming (hop-by-hop) form of `FirBank.convolve` (bsrnn_fir_stream_*): `rows` rows on `bank`, each on one filter of it or on
    -1 (bypass, where all rows start), each at its own place in its own stream.  A row that has taken N samples has been handed
    max(0, N // 1024 * 1024 - shift); flush() hands out the rest.  causal=False (shift = k // 2): a row's concatenated output, flush
    included, is `bank.convolve` of its concatenated input bit for bit, however the input is cut.  causal=True (shift = 0):
    y[m] = sum_j x[m - (k - 1) + j] h[j] - latency under one hop; give the bank a response reversed to convolve with it.  `max_taps`
    (default: the bank's largest filter) bounds the filters rows may be assigned.  One launch per call; made for ticks of many rows, and
    merely correct for many hops of few rows."""

    def __init__(self, bank, rows, max_taps=None, causal=False):
        if not isinstance(bank, FirBank):
            raise ValueError("FirStream: bank must be a FirBank, got %s" % type(bank).__name__)
        if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or rows < 1:
            raise ValueError("FirStream: rows must be a positive int, got %r" % (rows,))
        if max_taps is None:
            max_taps = max(bank.taps(i) for i in range(len(bank)))
        if isinstance(max_taps, bool) or not isinstance(max_taps, (int, np.integer)) or not 1 <= max_taps <= MAX_TAPS:
            raise ValueError("FirStream: max_taps must be an int in [1, %d], got %r" % (MAX_TAPS, max_taps))
        self.bank = bank                        # (the library keeps the bank alive too)
        self.C = int(rows)
        self.max_taps = int(max_taps)
        self.causal = bool(causal)
        self.device = bank.device
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_fir_stream_create(bank._h, self.C, self.max_taps, 1 if causal else 0, ctypes.byref(h)))
        self._h = h
        self._taken = [0] * self.C              # samples per row since the beginning of its stream, mirrored to size a flush's result

    def __del__(self):
        try:
            _lib.bsrnn_fir_stream_destroy(self._h)
        except Exception:
            pass

    def _rows(self, rows, who):
        if rows is None:
            rows = range(self.C)
        try:
            rows = list(rows)
        except TypeError:
            raise ValueError("FirStream.%s: rows must be a sequence of ints, got %s" % (who, type(rows).__name__)) from None
        for r in rows:
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)):
                raise ValueError("FirStream.%s: a row must be an int, got %s" % (who, type(r).__name__))
            if not 0 <= r < self.C:
                raise ValueError("FirStream.%s: row %d is outside [0, %d)" % (who, r, self.C))
        if len(set(rows)) != len(rows):
            raise ValueError("FirStream.%s: a row is listed twice in %s" % (who, rows))
        return [int(r) for r in rows], (ctypes.c_int32 * len(rows))(*rows)

    def assign(self, rows, filter):
        """The listed rows move to filter `filter` of the bank (-1: bypass) and start a new stream there (host only)."""
        if isinstance(filter, bool) or not isinstance(filter, (int, np.integer)) or not -1 <= filter < len(self.bank):
            raise ValueError("FirStream.assign: filter %r is outside [-1, %d)" % (filter, len(self.bank)))
        if filter >= 0 and self.bank.taps(filter) > self.max_taps:
            raise ValueError("FirStream.assign: filter %d has %d taps, the stream was made for max_taps = %d" % (
                filter, self.bank.taps(filter), self.max_taps))
        rows, arr = self._rows(rows, "assign")
        _check(_lib.bsrnn_fir_stream_assign(self._h, arr, len(rows), int(filter)))
        for r in rows:
            self._taken[r] = 0

    def filter_of(self, row):
        return int(_lib.bsrnn_fir_stream_filter_of(self._h, self._rows([row], "filter_of")[0][0]))

    def ready(self, row, n):
        """Samples the next process() would hand `row` if it gave the row n samples."""
        row = self._rows([row], "ready")[0][0]
        return int(_lib.bsrnn_fir_stream_ready(self._h, row, int(n)))

    def reset(self, rows=None):
        """The listed rows (default: all) forget their stream so far and start a new one on the filter they have (host only)."""
        rows, arr = self._rows(rows, "reset")
        _check(_lib.bsrnn_fir_stream_reset_rows(self._h, arr, len(rows)))
        for r in rows:
            self._taken[r] = 0

    def _out(self, out, want, who):
        width = max(want)
        if out is None:
            return torch.empty((self.C, width), device=self.device, dtype=torch.float32)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != self.device or out.dim() != 2
                or out.shape[0] != self.C or out.shape[1] < width or (out.stride(1) != 1 and out.shape[1] > 1)
                or (self.C > 1 and out.stride(0) < out.shape[1])):
            raise ValueError("FirStream.%s: out must be a float32 tensor [%d, >= %d] with contiguous rows that do not overlap on %s" % (
                who, self.C, width, self.device))
        return out

    def process(self, wave, counts=None, out=None):
        """wave [C, n] float32 on the stream's device, counts C ints in [0, n] (default: n for every row) -> (out, counts out): row r reads
        its first counts[r] samples and nothing behind them and is handed out[r, :counts_out[r]]; a given `out` is not written behind
        them, a new one is unspecified there.  A count of 0 holds the row.  Views with a row stride go by pointer, uncopied."""
        if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.shape[0] != self.C:
            raise ValueError("FirStream.process: expected wave [C = %d, n], got %s" % (
                self.C, tuple(wave.shape) if isinstance(wave, torch.Tensor) else type(wave).__name__))
        if wave.dtype != torch.float32:
            raise ValueError("FirStream.process: expected a float32 tensor, got %s" % wave.dtype)
        if not wave.is_cuda:
            raise _native.NativeError("FirStream.process: the waveform must be on a HIP device")
        if wave.device != self.device:
            raise ValueError("FirStream.process: the waveform is on %s, the stream on %s" % (wave.device, self.device))
        n = wave.shape[1]
        if counts is None:
            counts = [n] * self.C
        try:
            counts = list(counts.tolist() if isinstance(counts, (torch.Tensor, np.ndarray)) else counts)
        except TypeError:
            raise ValueError("FirStream.process: counts must be a sequence of %d ints, got %s" % (self.C, type(counts).__name__)) from None
        if len(counts) != self.C:
            raise ValueError("FirStream.process: %d counts for %d rows" % (len(counts), self.C))
        for r, c in enumerate(counts):
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= c <= n:
                raise ValueError("FirStream.process: row %d has count %r, need an int in [0, %d]" % (r, c, n))
        want = [int(_lib.bsrnn_fir_stream_ready(self._h, r, int(c))) for r, c in enumerate(counts)]
        n_in = (ctypes.c_int64 * self.C)(*[int(c) for c in counts])
        n_out = (ctypes.c_int64 * self.C)(*([-1] * self.C))
        with torch.cuda.device(self.device):
            if n > 0:
                w, w_stride = BSRNN._rows_view(wave.detach())
            else:
                w, w_stride = wave, 0
            out = self._out(out, want, "process")
            o_stride = out.stride(0) if self.C > 1 else max(out.shape[1], 1)
            _check(_lib.bsrnn_fir_stream_process(self._h, _ptr(w), w_stride, n_in, _ptr(out), o_stride, n_out, _stream_ptr(self.device)))
        got = list(n_out)
        assert got == want, (got, want)
        for r, c in enumerate(counts):
            self._taken[r] += int(c)
        return out, got

    def flush(self, rows=None, out=None):
        """The listed rows (default: all) are handed what they are still owed and start afresh; the others are untouched.
        -> (out [C, max count], the counts as a list: 0 for rows not listed)."""
        rows, arr = self._rows(rows, "flush")
        n_out = (ctypes.c_int64 * self.C)(*([-1] * self.C))
        # what a row is owed, from the mirrored count: everything it took less what it was handed (the library's counts are held against it)
        want = [0] * self.C
        for r in rows:
            f = self.filter_of(r)
            if f >= 0:
                shift = 0 if self.causal else self.bank.taps(f) // 2
                want[r] = self._taken[r] - max(0, self._taken[r] // 1024 * 1024 - shift)
        with torch.cuda.device(self.device):
            out = self._out(out, want, "flush")
            o_stride = out.stride(0) if self.C > 1 else max(out.shape[1], 1)
            _check(_lib.bsrnn_fir_stream_flush_rows(self._h, arr, len(rows), _ptr(out), o_stride, n_out, _stream_ptr(self.device)))
        got = list(n_out)
        assert got == want, (got, want)
        for r in rows:
            self._taken[r] = 0
        return out, got


def rir_draw(idx, n_rirs, channels_of, prob=0.1):
    """The reference's decisions for training clip `idx` (m_dataset.py:83-102), in its order, on a random.Random(idx) (the reference seeds
    the global generator with idx): the weighted choices([True, False]), choices(rirs), and one randint(0, C - 1) per ear, C =
    channels_of(rir) the channel count of the chosen response.  Returns None (no reverberation) or (rir, channel 1, channel 2)."""
    rng = random.Random(idx)
    if not rng.choices([True, False], weights=[prob, 1.0 - prob])[0]:
        return None
    rir = rng.choices(range(n_rirs))[0]
    c = channels_of(rir)
    return rir, rng.randint(0, c - 1), rng.randint(0, c - 1)


def reverb_pairs(bank, mixes, draws, chain=True):
    """Applies the drawn responses to the mixtures of an optimizer step, in place.  mixes: a list of [2, n] float32 tensors on the bank's
    device; draws: per clip None or (filter for row 0, filter for row 1) of `bank`.

    chain=True is the reference AS WRITTEN: row 0 becomes conv(a[0], rir1), and row 1 becomes conv(THAT RESULT, rir2) - m_dataset.py:111
    convolves a1 again, not a2, so the right channel of a reverberant clip is the left one under both responses.  chain=False convolves
    a[1] with rir2.  All chosen rows of the step go through ONE convolve call per stage (two with chain=True), not one per clip."""
    chosen = [i for i, d in enumerate(draws) if d is not None]
    if not chosen:
        return mixes
    n_max = max(mixes[i].shape[1] for i in chosen)
    dev = mixes[chosen[0]].device
    lens = [mixes[i].shape[1] for i in chosen]
    if chain:
        src = torch.zeros((len(chosen), n_max), device=dev, dtype=torch.float32)
        for j, i in enumerate(chosen):
            src[j, :lens[j]] = mixes[i][0]
        first = bank.convolve(src, lens, [draws[i][0] for i in chosen])
        second = bank.convolve(first, lens, [draws[i][1] for i in chosen])
        for j, i in enumerate(chosen):
            mixes[i][0] = first[j, :lens[j]]
            mixes[i][1] = second[j, :lens[j]]
        return mixes
    src = torch.zeros((2 * len(chosen), n_max), device=dev, dtype=torch.float32)
    for j, i in enumerate(chosen):
        src[2 * j:2 * j + 2, :lens[j]] = mixes[i]
    res = bank.convolve(src, [n for n in lens for _ in range(2)], [f for i in chosen for f in draws[i]])
    for j, i in enumerate(chosen):
        mixes[i][:] = res[2 * j:2 * j + 2, :lens[j]]
    return mixes


def _random_resize(x, length, rng):
    # m_dataset.py:123-139 (a clip of exactly `length` samples raises in randint(0, -1), as in the reference)
    if x.shape[1] < length:
        missing = length - x.shape[1]
        left = rng.randint(0, missing)
        z = torch.zeros((x.shape[0], 1), dtype=x.dtype)
        return torch.cat((z.repeat((1, left)).to(x.device), x, z.repeat((1, missing - left)).to(x.device)), dim=1)
    left = rng.randint(0, x.shape[1] - length - 1)
    return x[:, left:left + length]


def remix(dialog, backgrounds, length, rng):
    """MixDataSet.__getitem__'s arithmetic (m_dataset.py:158-178) on loaded tensors [ch, n], on their device: every background is
    random_resize'd to `length` (zero padding split at random, or a random cut), then scaled by uniform(0.1, 1.0); the dialog's scale is
    drawn and - as in the reference, where the multiplication is commented out - not applied; the dialog is resized; the mixture is
    dialog + sum(backgrounds).  `rng` (a random.Random, or the random module) is drawn from in the reference's order.  Returns
    (mixture, dialog)."""
    backgrounds = [_random_resize(x, length, rng) for x in backgrounds]
    backgrounds = [x * rng.uniform(0.1, 1.0) for x in backgrounds]
    rng.uniform(0.1, 1.0)                    # scale_dialog: drawn, unused
    dialog = _random_resize(dialog, length, rng)
    return dialog + sum(backgrounds), dialog


# ------------------------------------------------------------------------------------------ the re-mix on the device
# MixDataSet as a loader: the sources stay on the device (SourceShelf), the reference's draws are made on the host (remix_draw), and ONE
# bsrnn_remix_ragged writes the mixtures and targets of a whole optimizer step into the padded buffers train.train_loss_ragged takes
# (remix_many).  `remix` above is the oracle: same draws, same bits.
DIALOG, BACKGROUND = "dialog", "background"


class SourceShelf:
    """Dialog and background sources of a re-mixed training set, ALL held on `device` for as long as the shelf lives (a shelf larger than
    device memory is out of scope).  add_dialog / add_background take [n] or [ch, n] float32 tensors: CPU tensors are uploaded once; cuda
    tensors and views of them are kept by reference, uncopied, as long as their samples are contiguous.  A mono source serves both rows
    of a clip through the same pointer, as the reference's load_waveform duplicates it."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SourceShelf: the sources live on a HIP device, got %s" % (self.device,))
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._src = {DIALOG: [], BACKGROUND: []}            # per source its rows: 1-D tensors of contiguous samples on the device

    def _hold(self, t, who):
        if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.dtype != torch.float32 or t.shape[0] < 1:
            raise ValueError("SourceShelf.%s: expected a float32 tensor [n] or [ch, n], got %s" % (
                who, (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
        t = t.detach()
        if not t.is_cuda:
            t = t.to(self.device)
        elif t.device != self.device:
            raise ValueError("SourceShelf.%s: the tensor is on %s, the shelf on %s" % (who, t.device, self.device))
        if t.shape[-1] > 1 and t.stride(-1) != 1:
            t = t.contiguous()
        return t

    def _add(self, kind, t, who):
        t = self._hold(t, who)
        self._src[kind].append([t] if t.dim() == 1 else [t[c] for c in range(t.shape[0])])
        return len(self._src[kind]) - 1

    def add_dialog(self, t):
        return self._add(DIALOG, t, "add_dialog")

    def add_background(self, t):
        return self._add(BACKGROUND, t, "add_background")

    def add_sections(self, wave, sections):
        """The DIALOG / BACKGROUND sections `mining.mine` returned for the recording `wave` ([n] or [ch, n]), as views into it: the
        reference's section files receive the mixture's chunks (gendataset-separate.py), so the mined chain needs no copy and no file.
        `sections`: a `mining.Mined`, a list of `mining.Section` (all channels of `wave` are cut alike), or one such list per row of
        `wave` (every row a mono source of its own).  Returns (dialogs added, backgrounds added)."""
        from . import mining
        w = self._hold(wave, "add_sections")
        if hasattr(sections, "sections") and hasattr(sections, "activity"):
            sections = sections.sections
        sections = list(sections)
        per_row = bool(sections) and not hasattr(sections[0], "kind")
        if per_row and (w.dim() == 1 and len(sections) != 1 or w.dim() == 2 and len(sections) != w.shape[0]):
            raise ValueError("SourceShelf.add_sections: %d section lists for a recording %s" % (len(sections), tuple(w.shape)))
        added = {mining.DIALOG: 0, mining.BACKGROUND: 0}
        for r, secs in enumerate(sections if per_row else [sections]):
            for s in secs:
                a, b = s.samples
                if s.kind not in added or not 0 <= a < b <= w.shape[-1]:
                    raise ValueError("SourceShelf.add_sections: section %r does not lie in a recording of %d samples" % (s, w.shape[-1]))
                view = (w[r] if w.dim() == 2 else w)[a:b] if per_row else w[..., a:b]
                self._add(DIALOG if s.kind == mining.DIALOG else BACKGROUND, view, "add_sections")
                added[s.kind] += 1
        return added[mining.DIALOG], added[mining.BACKGROUND]

    @property
    def n_dialogs(self):
        return len(self._src[DIALOG])

    @property
    def n_backgrounds(self):
        return len(self._src[BACKGROUND])

    def __len__(self):
        return self.n_dialogs + self.n_backgrounds

    def _rows(self, kind, i):
        if kind not in self._src or isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < len(self._src[kind]):
            raise IndexError("SourceShelf: no %s %r (%s)" % (kind, i, ", ".join("%d %ss" % (len(v), k) for k, v in self._src.items())))
        return self._src[kind][i]

    def length_of(self, kind, i):
        return int(self._rows(kind, i)[0].shape[0])

    def channels_of(self, kind, i):
        return len(self._rows(kind, i))


class RemixSpec(NamedTuple):
    """What `remix_draw` decided for one item: the dialog, the backgrounds in order, and per term - the dialog first - where its sample 0
    lands in the item (`at` > 0: padding on the left, < 0: a cut) and its gain."""
    dialog: int
    backgrounds: tuple
    at: tuple
    gain: tuple
    length: int


def _resize_draw(n, length, rng):
    # random_resize's one draw (m_dataset.py:129-139) as the offset of the source in the item
    if n < length:
        return rng.randint(0, length - n)
    return -rng.randint(0, n - length - 1)                    # n == length: randint(0, -1) raises ValueError, as in the reference


def remix_draw(idx, shelf, length=50 * 44100, n_backgrounds=4, scale_dialog=False):
    """MixDataSet.__getitem__'s decisions for item `idx` (m_dataset.py:149-176), in its order, on a random.Random(idx) (the reference
    seeds the global generator with idx): two unused choice(backgrounds), four choice(dialogs) of which the first is used, n_backgrounds
    choice(backgrounds), one random_resize draw per background, one uniform(0.1, 1.0) per background, one for the dialog's scale - applied
    only with scale_dialog=True; the reference's multiplication is commented out - and the dialog's resize draw.  `shelf` is a SourceShelf,
    or anything with n_dialogs, n_backgrounds and length_of(kind, i).  A source of exactly `length` samples raises ValueError, as the
    reference's randint(0, -1) does."""
    if shelf.n_dialogs < 1 or shelf.n_backgrounds < 1:
        raise ValueError("remix_draw: the shelf holds %d dialogs and %d backgrounds, need at least one of each" % (shelf.n_dialogs, shelf.n_backgrounds))
    rng = random.Random(idx)
    dialogs, backgrounds = range(shelf.n_dialogs), range(shelf.n_backgrounds)
    rng.choice(backgrounds)
    rng.choice(backgrounds)
    dialog = rng.choice(dialogs)
    for _ in range(3):
        rng.choice(dialogs)
    bgs = [rng.choice(backgrounds) for _ in range(n_backgrounds)]
    at = [_resize_draw(shelf.length_of(BACKGROUND, b), length, rng) for b in bgs]
    gain = [rng.uniform(0.1, 1.0) for _ in bgs]
    scale = rng.uniform(0.1, 1.0)
    at.insert(0, _resize_draw(shelf.length_of(DIALOG, dialog), length, rng))
    gain.insert(0, scale if scale_dialog else 1.0)
    return RemixSpec(dialog, tuple(bgs), tuple(at), tuple(gain), int(length))


def remix_many(shelf, specs, length, out=None):
    """The items `specs` (RemixSpec, drawn for `length`) of one optimizer step in ONE bsrnn_remix_ragged: returns (mix [R, length],
    target [R, length], lengths, clip_rows) - the arguments of train.train_loss_ragged.  An item has the rows of its dialog (two for a
    mono one); a background has as many channels or is mono.  `out`: a (mix, target) pair of float32 [R, length] tensors on the
    shelf's device, which go by pointer with their row strides (contiguous samples, rows that do not overlap); all of both is written."""
    from . import train as _train
    specs = list(specs)
    length = int(length)
    if not specs or length < 1:
        raise ValueError("remix_many: need at least one spec and length >= 1")
    rows, terms, clip_rows = [], [], []
    for c, sp in enumerate(specs):
        if sp.length != length or len(sp.at) != 1 + len(sp.backgrounds) or len(sp.gain) != len(sp.at):
            raise ValueError("remix_many: spec %d was drawn for length %d with %d offsets and %d gains for %d terms, the call is for length %d" % (
                c, sp.length, len(sp.at), len(sp.gain), 1 + len(sp.backgrounds), length))
        srcs = [shelf._rows(DIALOG, sp.dialog)] + [shelf._rows(BACKGROUND, b) for b in sp.backgrounds]
        ch = max(2, len(srcs[0]))
        for t, s in enumerate(srcs):
            if len(s) not in (1, ch):
                raise ValueError("remix_many: spec %d: term %d has %d channels, the item %d" % (c, t, len(s), ch))
        for r in range(ch):
            rows.append((length, len(terms), len(srcs)))
            for s, at, g in zip(srcs, sp.at, sp.gain):
                x = s[r if len(s) > 1 else 0]
                terms.append((x.data_ptr() if x.shape[0] else None, x.shape[0], int(at), float(g), 0))
        clip_rows.append(ch)
    R = len(rows)
    dev = shelf.device
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty((R, length), device=dev, dtype=torch.float32), torch.empty((R, length), device=dev, dtype=torch.float32))
        for o in out:
            if (not isinstance(o, torch.Tensor) or o.dtype != torch.float32 or o.device != dev or tuple(o.shape) != (R, length)
                    or (o.stride(1) != 1 and length > 1) or (R > 1 and o.stride(0) < length)):
                raise ValueError("remix_many: out must be two float32 tensors %s with contiguous rows that do not overlap on %s" % ((R, length), dev))
        mix, target = out
        _check(_lib.bsrnn_remix_ragged(_train._context(dev), (_native.RemixRowC * R)(*rows), R, (_native.RemixTermC * len(terms))(*terms), len(terms),
                                       _ptr(mix), mix.stride(0) if R > 1 else length, _ptr(target), target.stride(0) if R > 1 else length,
                                       length, _stream_ptr(dev)))
    return mix, target, [length] * len(specs), clip_rows
