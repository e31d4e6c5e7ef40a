"""Dialog / background section mining: the reference's gendataset-separate.py on the device.

The reference runs its separator over a long recording, forms a dialog-to-background figure and a level for every hop of 1024 samples
(gendataset-separate.py:100-109) and cuts the recording into dialog and background sections with a run-length state machine (:111-149).
`hop_activity` forms the two figures for a ragged batch in one kernel launch (include/bsrnn_hip.h, bsrnn_hop_activity), `SectionScanner`
is the state machine (bsrnn_sections_scan, a host function of the library), `mine` runs a shelf of recordings of unequal length through
`BSRNN.separate_long_ragged`, `hop_activity` and the scanner: one separation, one activity launch and one download per bucket.
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _native
from . import spec as _spec
from .bsrnn import BSRNN, _ptr, _stream_ptr

_lib = _native.lib
_check = _native.check
HOP = _spec.HOP
RATIO, LEVEL = _native.ACT_RATIO, _native.ACT_LEVEL
DIALOG, BACKGROUND = _native.SECTION_DIALOG, _native.SECTION_BACKGROUND
KIND_NAMES = {DIALOG: "dialog", BACKGROUND: "background"}


def hop_activity(model, mix, est, hops=None, out=None):
    """mix [R, n_mix], est [R, n_est] float32 on a HIP device -> float64 [R, H, 2] on that device, H = min(n_mix, n_est) // 1024:
    [r, h, 0] = mean(e^2 / (w - e)^2) and [r, h, 1] = mean(w^2) over hop h of row r (w the mixture, e the estimate; fp32 terms as the
    reference forms them, double sums).  Raw means, not dB.  hops[r] <= H, if given, is row r's hop count: nothing behind hops[r] * 1024
    samples of a row is read and the slots from hops[r] on hold (0, 0).  Views with a row stride (buf[:, a:b], a channel slice) go by
    pointer and stride, uncopied - a comparison against later or earlier input is such a slice.  `out`: a contiguous float64 [R, H, 2]."""
    for name, t in (("mix", mix), ("est", est)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
            raise ValueError("hop_activity: %s must be a 2-D float32 tensor, got %s" % (
                name, "%s %s" % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
        if not t.is_cuda:
            raise _native.NativeError("hop_activity: %s must be on a HIP device" % name)
    if mix.device != est.device or mix.shape[0] != est.shape[0]:
        raise ValueError("hop_activity: mix %s on %s and est %s on %s must have the same rows on one device" % (
            tuple(mix.shape), mix.device, tuple(est.shape), est.device))
    R, H = mix.shape[0], min(mix.shape[1], est.shape[1]) // HOP
    if R < 1 or H < 1:
        raise ValueError("hop_activity: need at least one row and one hop of 1024 samples, got mix %s, est %s" % (tuple(mix.shape), tuple(est.shape)))
    counts = None
    if hops is not None:
        counts = [int(h) for h in hops]
        if len(counts) != R:
            raise ValueError("hop_activity: %d hop counts for %d rows" % (len(counts), R))
        for r, h in enumerate(counts):
            if not 0 <= h <= H:
                raise ValueError("hop_activity: row %d has %d hops, need 0 <= hops <= %d" % (r, h, H))
    dev = mix.device
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != dev
                            or tuple(out.shape) != (R, H, 2) or not out.is_contiguous()):
        raise ValueError("hop_activity: out must be a contiguous float64 tensor %s on %s" % ((R, H, 2), dev))
    w, w_stride = BSRNN._rows_view(mix.detach())
    e, e_stride = BSRNN._rows_view(est.detach())
    with torch.cuda.device(dev):
        ctx = model._context(dev)
        if out is None:
            out = torch.empty((R, H, 2), device=dev, dtype=torch.float64)
        _check(_lib.bsrnn_hop_activity(ctx, _ptr(w), w_stride, _ptr(e), e_stride, (ctypes.c_int32 * R)(*counts) if counts is not None else None,
                                       R, H, _ptr(out), _stream_ptr(dev)))
    return out


class SectionRule:
    """The thresholds of the state machine (bsrnn_section_rule); the defaults are the reference's constants
    (gendataset-separate.py:106-138): dialog above 10, bridge above 3, background below -30, silence below -100 (10 ln of the two means),
    a level mean below 1e-10 counts as -200, and a section opens at the 10th hop of a run."""
    FIELDS = ("dialog_db", "bridge_db", "background_db", "silence_db", "level_floor", "floor_db", "min_run")

    def __init__(self, **kw):
        c = _native.SectionRuleC()
        _lib.bsrnn_section_rule_default(ctypes.byref(c))
        for k in self.FIELDS:
            setattr(self, k, getattr(c, k))
        for k, v in kw.items():
            if k not in self.FIELDS:
                raise TypeError("SectionRule: unknown field %r (fields: %s)" % (k, ", ".join(self.FIELDS)))
            setattr(self, k, int(v) if k == "min_run" else float(v))
        if self.min_run < 1:
            raise ValueError("SectionRule: min_run = %d, need at least 1" % self.min_run)

    def _c(self):
        return _native.SectionRuleC(*[getattr(self, k) for k in self.FIELDS])

    def __repr__(self):
        return "SectionRule(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.FIELDS)


class Section(NamedTuple):
    """A closed section: kind (DIALOG = 1, BACKGROUND = 2), first_hop, end_hop (exclusive), in hops since the scanner's reset."""
    kind: int
    first_hop: int
    end_hop: int

    @property
    def samples(self):
        return (self.first_hop * HOP, self.end_hop * HOP)

    @property
    def name(self):
        return KIND_NAMES[self.kind]


class SectionScanner:
    """The run-length state machine of gendataset-separate.py:111-149 over per-hop activity, a thin wrapper over the library's state
    (bsrnn_section_state, bsrnn_sections_scan; the rule is spelled out in include/bsrnn_hip.h).  feed(act) consumes hops [n, 2] - one
    row of a downloaded `hop_activity` - and returns the sections they close; flush() closes an open section at the end of the audio.
    Feeding a stream in any split gives the sections of one feed.  A ratio of exactly 0 counts as -inf dB (the reference's math.log
    raises there)."""

    def __init__(self, rule=None):
        if rule is not None and not isinstance(rule, SectionRule):
            raise ValueError("SectionScanner: rule must be a SectionRule, got %s" % type(rule).__name__)
        self.rule = rule if rule is not None else SectionRule()
        self._state = _native.SectionStateC()
        self.reset()

    def reset(self):
        _lib.bsrnn_section_state_reset(ctypes.byref(self._state))

    @property
    def hop(self):
        """Hops consumed since the last reset."""
        return int(self._state.hop)

    @property
    def open(self):
        """(kind, first_hop) of the open section, or None."""
        return (int(self._state.open_kind), int(self._state.open_hop)) if self._state.open_kind else None

    def _scan(self, a, flush):
        n = a.shape[0]
        cap = n + 1                                 # a hop closes at most one section, the flush one more
        out = (_native.SectionC * cap)()
        got = ctypes.c_int64()
        rule = self.rule._c()
        _check(_lib.bsrnn_sections_scan(ctypes.byref(rule), ctypes.byref(self._state), a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if n else None,
                                        n, 1 if flush else 0, out, cap, ctypes.byref(got)))
        return [Section(int(s.kind), int(s.first_hop), int(s.end_hop)) for s in out[:got.value]]

    def feed(self, act, flush=False):
        a = act.detach().cpu().numpy() if isinstance(act, torch.Tensor) else np.asarray(act)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("SectionScanner.feed: expected activity [n, 2], got %s" % (a.shape,))
        return self._scan(np.ascontiguousarray(a, dtype=np.float64), flush)

    def flush(self):
        return self._scan(np.empty((0, 2), np.float64), True)


class Mined(NamedTuple):
    """What `mine` returns per clip: sections[row] the row's closed sections, activity [rows, n // 1024, 2] (numpy float64)."""
    sections: list
    activity: np.ndarray


def mine(model, clips, segment_frames=256, max_rows=64, rule=None):
    """Where is the dialog: clips as `BSRNN.separate_many_long` takes them (1-D [n] or 2-D [ch, n] tensors, n > 1024, on the GPU or the
    CPU).  Every row (channel) is a stream of its own, as with the reference's --channel.  `spec.long_buckets` groups the clips; per
    bucket there is ONE `separate_long_ragged`, ONE `hop_activity` with hops[r] = n_r // 1024 and one download of the activity; the
    scanner then runs on the host, per row, flushed at the row's end.  The estimate and the mixture are compared ALIGNED (the reference's
    loop compares its delayed stream output with the current chunk; see include/bsrnn_hip.h).  Returns, per clip in input order, a
    `Mined(sections, activity)`: sections[row] a list of `Section`, activity [rows, n // 1024, 2]."""
    clips = list(clips)
    for i, c in enumerate(clips):
        if not isinstance(c, torch.Tensor) or c.dim() not in (1, 2) or c.shape[-1] <= HOP or c.shape[0] < 1:
            raise ValueError("mine: clip %d must be a tensor [n] or [ch, n] with n > 1024, got %s" % (
                i, tuple(c.shape) if isinstance(c, torch.Tensor) else type(c).__name__))
    if rule is not None and not isinstance(rule, SectionRule):
        raise ValueError("mine: rule must be a SectionRule, got %s" % type(rule).__name__)
    seg = int(segment_frames)
    if seg < 1:
        raise ValueError("mine: segment_frames = %d (at least one frame per segment)" % seg)
    buckets = _spec.long_buckets([_spec.n_frames(c.shape[-1]) for c in clips], [1 if c.dim() == 1 else c.shape[0] for c in clips], max_rows)
    if not clips:
        return []
    dev = next((c.device for c in clips if c.is_cuda), None) or model._device_for(clips[0])
    scanner = SectionScanner(rule)
    results = [None] * len(clips)
    for bucket in buckets:
        rows = [1 if clips[i].dim() == 1 else clips[i].shape[0] for i in bucket]
        lens = [clips[i].shape[-1] for i in bucket]
        buf = torch.empty((sum(rows), max(lens)), device=dev, dtype=torch.float32)      # (behind a row's end nothing is read)
        r0 = 0
        for i, ch, n in zip(bucket, rows, lens):
            buf[r0:r0 + ch, :n] = clips[i].detach().reshape(ch, n).to(device=dev, dtype=torch.float32)
            r0 += ch
        row_lens = [n for ch, n in zip(rows, lens) for _ in range(ch)]
        est = model.separate_long_ragged(buf, row_lens, seg)
        act = hop_activity(model, buf, est, hops=[n // HOP for n in row_lens]).cpu().numpy()      # the one download
        r0 = 0
        for i, ch, n in zip(bucket, rows, lens):
            a = np.ascontiguousarray(act[r0:r0 + ch, :n // HOP])
            sections = []
            for r in range(ch):
                scanner.reset()
                sections.append(scanner.feed(a[r], flush=True))
            results[i] = Mined(sections, a)
            r0 += ch
    return results
