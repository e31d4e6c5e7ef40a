"""Session pools: many live sessions on one wide stream.  StreamPool packs them around a StreamingSeparator in Python; NativeStreamPool
and NativeRatePool are the library's object (bsrnn_pool_*), one call per tick.  The three share one session table and one set of
argument checks, _SessionPool.  `from speechseparation_amd.bsrnn import StreamPool, NativeStreamPool, NativeRatePool` gives the same
classes."""
import ctypes

import numpy as np
import torch

from . import _native
from . import spec as _spec
from .bsrnn import _check, _lib, _stream_ptr
from .resample import ResamplerBank, resample_len
from .streaming import StreamingSeparator, look_at_weights, row_floats


class _SessionPool:
    """What the pools have in common, none of it needing a device: `slots` sessions of `rows` rows each, the lowest free slot for a new
    one, a sample rate per session for the pools that have `rates`, and the checks of what feed, step, drain and adopt are given.
    Every check takes the name it refuses under (`who`, as in "NativeStreamPool.step"): a NativeRatePool that inherits feed, step
    and adopt refuses under NativeStreamPool's name."""

    MODEL_RATE = 44100

    def __init__(self, who, model, slots, rows_per_session, device, **more):
        for name, v in (("slots", slots), ("rows_per_session", rows_per_session)) + tuple(more.items()):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("%s: %s must be a positive int, got %r" % (who, name, v))
        if slots * rows_per_session > _native.STREAM_ROWS_MAX:
            raise ValueError("%s: %d slots x %d rows is more than the %d rows a rows call takes" % (
                who, slots, rows_per_session, _native.STREAM_ROWS_MAX))
        self.model, self.slots, self.rows, self._device = model, int(slots), int(rows_per_session), device
        self._slot = {}                     # session id -> slot
        self._free = list(range(self.slots))
        self._next = 0
        self.rates = None                   # the pool's session rates, for the pools that take them
        self._rate = {}                     # session id -> index into rates, for the sessions that have one

    # ------------------------------------------------------------------ slots
    def _rows_of(self, sid):
        slot = self._slot[sid]              # KeyError: no such session
        return range(slot * self.rows, (slot + 1) * self.rows)

    def sessions(self):
        return list(self._slot)

    def _check_free(self, who):
        if not self._free:
            raise ValueError("%s: all %d slots are in use" % (who, self.slots))

    def _take_slot(self, who):
        """-> a new session's id, on the lowest free slot."""
        self._check_free(who)
        sid, self._next = self._next, self._next + 1
        self._slot[sid] = self._free.pop(0)
        return sid

    def _give_slot(self, sid):
        """The session leaves, its rate with it -> the slot it had."""
        slot = self._slot.pop(sid)
        self._free.append(slot)
        self._free.sort()
        self._rate.pop(sid, None)
        return slot

    # ------------------------------------------------------------------ rates
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

    def _rate_index(self, sample_rate, who):
        """open()'s sample_rate -> its index into the pool's rates, None for a session at the model's rate."""
        if sample_rate is None or sample_rate == self.MODEL_RATE:
            return None
        if self.rates is None or sample_rate not in self.rates:
            raise ValueError("%s: sample_rate %r is not one of the pool's rates %r" % (who, sample_rate, self.rates))
        return self.rates.index(sample_rate)

    def rate_of(self, sid):
        """The session's sample rate (44100 for one opened without)."""
        self._rows_of(sid)
        return self.rates[self._rate[sid]] if sid in self._rate else self.MODEL_RATE

    def _check_steps(self, sid, who):
        if sid in self._rate:
            raise ValueError("%s: session %r has a sample rate of its own (%d Hz): its audio does not come in whole hops, "
                             "use feed()" % (who, sid, self.rates[self._rate[sid]]))

    def _check_moves(self, sid, who):
        if sid in self._rate:
            raise ValueError("%s: session %r has a sample rate of its own (%d Hz); the resamplers' carries do not move "
                             "with a session" % (who, sid, self.rates[self._rate[sid]]))

    # ------------------------------------------------------------------ what the calls are given
    def _check_dict(self, chunks, who):
        if not isinstance(chunks, dict):
            raise ValueError("%s: chunks must be a dict {session id: tensor}, got %s" % (who, type(chunks).__name__))

    def _check_chunk(self, sid, t, who, n):
        """A known session and a tensor of its rows; `n` is how the message writes the samples per row."""
        self._rows_of(sid)
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != self.rows:
            raise ValueError("%s: session %r needs a tensor [%d, %s], got %s" % (
                who, sid, self.rows, n, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))

    def _check_chunks(self, chunks, who):
        """feed's form: any n, another one per session."""
        self._check_dict(chunks, who)
        for sid, t in chunks.items():
            self._check_chunk(sid, t, who, "n")

    def _check_hop_chunks(self, chunks, who):
        """step's form: whole hops, one L for all, sessions at the model's rate -> the samples per row (None for an empty dict)."""
        self._check_dict(chunks, who)
        n = None
        for sid, t in chunks.items():
            self._check_chunk(sid, t, who, "L*1024")
            if t.shape[1] % _spec.HOP or t.shape[1] == 0:
                raise ValueError("%s: session %r holds %d samples per row, need whole hops of 1024" % (who, sid, t.shape[1]))
            if n is not None and t.shape[1] != n:
                raise ValueError("%s: session %r holds %d samples per row, the others %d (one L per step)" % (who, sid, t.shape[1], n))
            n = t.shape[1]
            self._check_steps(sid, who)
        return n

    def _check_mix(self, mix, who):
        """feed's and step's form: None, one float, or {session id: float}."""
        if isinstance(mix, dict):
            for sid, v in mix.items():
                self._rows_of(sid)
                if isinstance(v, bool) or not isinstance(v, (int, float)):
                    raise ValueError("%s: mix of session %r must be a float, got %s" % (who, sid, type(v).__name__))
        elif mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("%s: mix must be None, a float or a dict {session id: float}, got %s" % (who, type(mix).__name__))

    def _check_one_mix(self, mix, who):
        """drain's form: None or one float."""
        if mix is not None and (isinstance(mix, bool) or not isinstance(mix, (int, float))):
            raise ValueError("%s: mix must be None or a float, got %s" % (who, type(mix).__name__))

    def _row_floats(self):
        return row_floats(self.model)

    def _check_blobs(self, blobs, who):
        """adopt's blobs, one per row -> as a list."""
        blobs = list(blobs)
        nf = self._row_floats()
        if len(blobs) != self.rows or not all(isinstance(b, torch.Tensor) and b.dim() == 1 and b.numel() == nf for b in blobs):
            raise ValueError("%s: need %d blobs of %d floats each" % (who, self.rows, nf))
        return blobs


class StreamPool(_SessionPool):
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

    def __init__(self, model, slots, rows_per_session=1, device=None, rates=None):
        rates = self._checked_rates(rates)              # (checked before anything else)
        super().__init__("StreamPool", model, slots, rows_per_session, device)
        self.rates = rates
        self._st = None
        self._pend = {}                     # feed(): session id -> the samples (fewer than one hop) that wait for its next feed
        self._skip = {}                     # a session with a rate -> samples of the stream's delay still to be dropped from its output
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

    def open(self, sample_rate=None):
        """-> a new session's id; its rows start from silence.  sample_rate: None or the model's 44100 for a session that gives and gets
        audio at the model's rate, else one of the pool's `rates`.  ValueError when every slot is taken or the rate is not one of them."""
        k = self._rate_index(sample_rate, "StreamPool.open")
        sid = self._take_slot("StreamPool")
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
        if sid in self._rate and self._bank_in is not None:
            self._bank_in.reset_rows(rows)
            self._bank_out.reset_rows(rows)
        self._skip.pop(sid, None)
        self._give_slot(sid)
        self._pend.pop(sid, None)

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
        self._check_chunks(chunks, "StreamPool.feed")
        self._check_mix(mix, "StreamPool.feed")
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

    def _packed(self, blocks, n, marks, mix):
        """The sessions' audio as the wide stream takes it: blocks {sid: float32 tensor [rows_per_session, up to n] on the stream's device}
        and marks {sid: a value for each of its rows} -> (wave [C, n] with zeros where nobody wrote, the marks per row with 0 for the
        rows of nobody, the mix argument of the rows calls)."""
        st = self._st
        C = self.slots * self.rows
        wave = torch.zeros((C, n), dtype=torch.float32, device=st.device)
        per_row = isinstance(mix, dict)
        row_marks = [0] * C
        mix_rows = [1.0] * C
        for sid, t in blocks.items():
            rows = self._rows_of(sid)
            wave[rows.start:rows.stop, :t.shape[1]] = t
            for r in rows:
                row_marks[r] = marks[sid]
                if per_row:
                    mix_rows[r] = float(mix.get(sid, 1.0))
        m = torch.tensor(mix_rows, dtype=torch.float32) if per_row else (1.0 if mix is None else float(mix))
        return wave, row_marks, m

    def _feed_hops(self, chunks, mix):
        """feed() behind its argument checks, for chunks at the model's rate."""
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
        while any(have[sid] // hop > done[sid] for sid in chunks):
            take = {sid: min(have[sid] // hop - done[sid], _native.STREAM_HOPS_MAX) for sid in chunks}
            blocks = {sid: audio[sid][:, done[sid] * hop:(done[sid] + h) * hop] for sid, h in take.items()}
            wave, counts, m = self._packed(blocks, max(take.values()) * hop, take, mix)
            out = self._st.process_hops(wave, counts, m)
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
        n = self._check_hop_chunks(chunks, "StreamPool.step")
        self._check_mix(mix, "StreamPool.step")
        if not chunks:
            return {}
        st = self._stream()
        staged = {sid: t.detach().to(device=st.device, dtype=torch.float32) for sid, t in chunks.items()}
        wave, active, m = self._packed(staged, n, dict.fromkeys(chunks, True), mix)
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
        self._check_moves(sid, "StreamPool.export")
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
        self._check_one_mix(mix, "StreamPool.drain")
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
        blobs = self._check_blobs(blobs, "StreamPool.adopt")
        self._check_free("StreamPool")
        st = self._stream()
        sid = self.open()
        for r, b in zip(self._rows_of(sid), blobs):
            st.set_row(r, b)
        return sid


class NativeStreamPool(_SessionPool):
    """StreamPool's sessions at the model's rate as an object of the LIBRARY (bsrnn_pool_*, include/bsrnn_hip.h): the slots, the samples
    that wait for a whole hop (a device-resident FIFO per row) and the packing of every session's audio around the one
    bsrnn_stream_process_hops of a tick all live behind ONE library call per feed, which takes a pointer per session.  Nothing is
    copied on the host: a CUDA chunk goes by its pointer and row stride (views are fine; float32 with unit inner stride), and the
    results are views of one tensor allocated per feed.  A dict of CPU tensors takes the library's host form (bsrnn_pool_feed_host).
    Same numbers as StreamPool: both make the same hops calls on the same samples (a feed of more than max_hops hops runs in rounds of
    max_hops, where StreamPool's rounds are 255 hops long).  The pool is created at the first call that needs the device; shape and
    type errors are raised before that.  Sessions with a sample rate of their own: the subclass NativeRatePool (or StreamPool(rates=...))."""

    _NAME = "NativeStreamPool"              # what open() refuses under; the subclass has its own

    def __init__(self, model, slots, rows_per_session=1, device=None, max_hops=8):
        super().__init__("NativeStreamPool", model, slots, rows_per_session, device, max_hops=max_hops)
        if max_hops > _native.STREAM_HOPS_MAX:
            raise ValueError("NativeStreamPool: max_hops = %d, a hops call takes at most %d" % (max_hops, _native.STREAM_HOPS_MAX))
        self.max_hops = int(max_hops)
        self.device = None                  # set with the pool
        self._h = None
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

    def open(self, sample_rate=None):
        """-> a new session's id; its rows start from silence and nothing waits.  sample_rate: None or the model's 44100 for a session
        at the model's rate, else - in a pool that has them, NativeRatePool - one of the pool's `rates`.  ValueError when every slot is
        taken or the rate is not one of them; a pool without rates refuses every other sample_rate."""
        if self.rates is None and sample_rate is not None and sample_rate != self.MODEL_RATE:
            raise ValueError("NativeStreamPool.open: sample_rate %r: the native pool serves sessions at the model's %d Hz; sessions with a "
                             "rate of their own are StreamPool(rates=...)'s" % (sample_rate, self.MODEL_RATE))
        k = self._rate_index(sample_rate, self._NAME + ".open")
        sid = self._take_slot(self._NAME)
        if k is not None:
            self._rate[sid] = k
        if self._h is not None:
            slot = self._slot[sid]
            got = ctypes.c_int32()
            with torch.cuda.device(self.device):
                self._open_slot(self._h, slot, got)
            assert got.value == slot
        return sid

    def close(self, sid):
        """The session leaves; samples of it that waited are dropped, and its rows of the resampler banks (a pool with rates) start afresh."""
        slot = self._give_slot(sid)
        if self._h is not None:
            _check(_lib.bsrnn_pool_close(self._h, slot))

    def pending(self, sid):
        """Samples per row of the session that wait for its next feed() (fewer than one hop)."""
        slot = self._slot[sid]
        return 0 if self._h is None else int(_lib.bsrnn_pool_pending(self._h, slot))

    def feed(self, chunks, mix=None):
        """chunks {sid: tensor [rows_per_session, n]}, ANY n >= 0 and another one per session, all CUDA tensors on the pool's device or all
        CPU tensors -> {sid: tensor [rows_per_session, h*1024] on the same device}: every session advances by the h = (pending + n) //
        1024 hops it has in hand, in ONE library call (bsrnn_pool_feed / _feed_host); the remainder waits on the device.  Sessions not
        named are held.  mix: None (1.0), one float, or {sid: float} (sessions not in it: 1.0).  The chunks must be float32 with unit
        inner stride (a row stride of any size: column slices and views with a storage offset go by pointer, uncopied); the results
        are views of one tensor made by this call."""
        self._check_dict(chunks, "NativeStreamPool.feed")
        on_cuda = None
        for sid, t in chunks.items():
            self._check_chunk(sid, t, "NativeStreamPool.feed", "n")
            if t.dtype != torch.float32:
                raise ValueError("NativeStreamPool.feed: session %r needs float32 samples, got %s (the chunk goes by pointer)" % (sid, t.dtype))
            n = t.shape[1]
            if n and (t.stride(1) != 1 or (self.rows > 1 and t.stride(0) < n)):
                raise ValueError("NativeStreamPool.feed: session %r: strides %r; the chunk goes by pointer and row stride, so samples of a row "
                                 "must be adjacent and rows must not overlap" % (sid, tuple(t.stride())))
            if on_cuda is not None and t.is_cuda != on_cuda:
                raise ValueError("NativeStreamPool.feed: CUDA and CPU chunks in one call; a feed takes one kind")
            on_cuda = t.is_cuda
        self._check_mix(mix, "NativeStreamPool.feed")
        if not chunks:
            return {}
        h = self._pool()
        for sid, t in chunks.items():
            if t.is_cuda and t.device != self.device:
                raise ValueError("NativeStreamPool.feed: session %r brings a chunk on %s, the pool lives on %s" % (sid, t.device, self.device))
        look_at_weights(self)
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
        self._check_hop_chunks(chunks, "NativeStreamPool.step")
        self._check_mix(mix, "NativeStreamPool.step")
        return self.feed(chunks, mix)

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
        blobs = self._check_blobs(blobs, "NativeStreamPool.adopt")
        if pending is not None and (not isinstance(pending, torch.Tensor) or pending.dim() != 2 or pending.shape[0] != self.rows or
                                    pending.shape[1] >= _spec.HOP):
            raise ValueError("NativeStreamPool.adopt: pending must be a tensor [%d, n] with n < %d, got %s" % (
                self.rows, _spec.HOP, tuple(pending.shape) if isinstance(pending, torch.Tensor) else type(pending).__name__))
        self._check_free("NativeStreamPool")
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

    _NAME = "NativeRatePool"

    def __init__(self, model, slots, rows_per_session=1, device=None, max_hops=8, rates=(48000,), max_block=48000):
        rates = self._checked_rates(rates)
        if rates is None:
            raise ValueError("NativeRatePool: rates must be a tuple of sample rates, got None (a pool without is NativeStreamPool)")
        if isinstance(max_block, bool) or not isinstance(max_block, (int, np.integer)) or not 1 <= max_block <= 1 << 24:
            raise ValueError("NativeRatePool: max_block must be an int in [1, 2^24], got %r" % (max_block,))
        super().__init__(model, slots, rows_per_session, device, max_hops)
        self.rates, self.max_block = rates, int(max_block)

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
                self._check_steps(sid, "NativeRatePool.step")
        return super().step(chunks, mix)

    def export(self, sid):
        """NativeStreamPool.export, for a session at the model's rate."""
        self._rows_of(sid)
        self._check_moves(sid, "NativeRatePool.export")
        return super().export(sid)

    def drain(self, sid, mix=None):
        """The session's audio ends: -> the tail it is still owed, [rows_per_session, n] on the pool's device, at the session's rate -
        StreamPool.drain's steps and its LENGTH rule, in one library call (bsrnn_pool_drain).  The session stays open and its next feed()
        begins a new piece of audio.  mix: None or one float."""
        slot = self._slot[sid]
        self._check_one_mix(mix, "NativeRatePool.drain")
        h = self._pool()
        look_at_weights(self)
        n = int(_lib.bsrnn_pool_drain_len(h, slot))
        out = torch.empty((self.rows, n), dtype=torch.float32, device=self.device)
        got = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _check(_lib.bsrnn_pool_drain(h, slot, out.data_ptr() if n else None, n, ctypes.byref(got), 1.0 if mix is None else float(mix),
                                         _stream_ptr(self.device)))
        assert got.value == n
        return out
