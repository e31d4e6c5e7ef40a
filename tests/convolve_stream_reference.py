"""The streaming FIR convolution's reference (bsrnn_fir_stream_*), shared by tests/test_convolve_stream_host.py (CPU) and
tests/test_gpu_convolve_stream.py.  No test lives here.

`plan` restates csrc/convolve_stream_host.h by brute force.  `StreamModel` is the scheme in float32 with per-frame torch.fft on the CPU: a
ring of P spectra, blocks formed as their frame completes, partitions summed ascending, the flush rule of convolve_host.h (frames behind f1
are neither analysed nor read).  Under the SAME alignment it equals convolve_reference.ref32 bit for bit for every cutting; under the
CAUSAL alignment it is the float32 reference (e_f32) of the GPU tests."""
import numpy as np
import torch

import convolve_reference as cr

B = cr.B
SAME, CAUSAL = 0, 1
DRAW = (0, 1, 1023, 1024, 1025, 3000)


def shift_of(k, align):
    return 0 if align == CAUSAL else k // 2


def emitted(N, shift):
    """Output samples a row that took N has been handed: those of the complete blocks, moved left by shift."""
    return max(0, N // B * B - shift)


def cuttings(n, seed):
    """The three ways of cutting n samples into calls: all at once, hop by hop, and a seeded ragged draw (counts of 0 included)."""
    rng = np.random.default_rng(seed)
    ragged, at = [], 0
    while at < n:
        c = min(int(rng.choice(DRAW)), n - at)
        ragged.append(c)
        at += c
    return {"once": [n], "hops": [min(B, n - a) for a in range(0, n, B)], "ragged": ragged}


def plan(k, align, cuts):
    """Brute force, from the definition alone: per call (first block, blocks, ready), and the flush (u1, f1, n_out)."""
    shift = shift_of(k, align)
    N, calls = 0, []
    for c in cuts:
        done = [u for u in range((N + c) // B + 1) if (u + 1) * B <= N + c and not (u + 1) * B <= N]      # frames this call completes
        out = [m for m in range(max(0, N - shift - B), N + c) if (m + shift) // B in done]                  # y[m] lies in block (m + shift) // B
        calls.append((N // B, len(done), len(out)))
        N += c
    handed = sum(c[2] for c in calls)
    if N == 0:
        return calls, (-1, -1, 0)
    u1 = (N - 1 + shift) // B
    f1 = min(u1, max(v for v in range(u1 + 2) if (v - 1) * B + 1 <= N - 1))      # the last frame that holds a sample of the row behind its sample 0
    return calls, (u1, f1, N - handed)


class StreamModel:
    """One row under the filter h.  process(x) -> the samples handed out, flush() -> the rest; both float32 arrays."""

    def __init__(self, h, align=SAME):
        h = np.asarray(h, np.float32)
        self.k = h.shape[0]
        self.P, self.shift = -(-self.k // B), shift_of(self.k, align)
        self.u0 = self.shift // B
        g = np.zeros(self.P * B, np.float32)
        g[:self.k] = h[::-1]
        part = np.zeros((self.P, 2 * B), np.float32)
        part[:, :B] = g.reshape(self.P, B)
        self.H = torch.fft.rfft(torch.from_numpy(part), dim=1)                  # complex64 [P, 1025], as ref32's
        self.ring = torch.zeros((self.P, B + 1), dtype=torch.complex64)
        self.reset()

    def reset(self):
        # host only: nothing of the ring, the tail or the FIFO is cleared - a new stream must not read what an old one left
        self.N = 0
        self.tail = getattr(self, "tail", np.full(B, np.nan, np.float32))
        self.fifo = np.zeros(0, np.float32)
        self.writes = {}                                                         # ring slot -> frame, to catch a slot overwritten too early

    def _analyse(self, u, block):
        prev = self.tail if u > 0 else np.zeros(B, np.float32)                   # zeros in front of the stream, whatever the tail holds
        frame = np.concatenate((prev, block)).astype(np.float32)
        self.ring[u % self.P] = torch.fft.rfft(torch.from_numpy(frame)[None, :], dim=1)[0]
        self.writes[u % self.P] = u
        self.tail = block

    def _form(self, u, f1, n_end):
        Y = torch.zeros((1, B + 1), dtype=torch.complex64)
        for p in range(min(self.P - 1, u) + 1):                                  # ascending; a frame behind f1 adds nothing
            v = u - p
            if v > f1:
                continue
            assert self.writes.get(v % self.P) == v, (u, p)
            Y[0] += self.ring[v % self.P] * self.H[p]
        y = torch.fft.irfft(Y, n=2 * B, dim=1)[0, B:].numpy()
        m0 = u * B - self.shift
        a, b = max(0, m0), min(m0 + B, n_end)
        return y[a - m0:b - m0].astype(np.float32)

    def process(self, x):
        x = np.asarray(x, np.float32)
        buf = np.concatenate((self.fifo, x))
        out = []
        u = self.N // B
        while buf.shape[0] >= B:
            self._analyse(u, buf[:B].copy())
            buf = buf[B:]
            if u >= self.u0:
                out.append(self._form(u, 1 << 60, 1 << 60))
            u += 1
        self.fifo = buf.copy()
        self.N += x.shape[0]
        return np.concatenate(out) if out else np.zeros(0, np.float32)

    def flush(self):
        n = self.N
        out = []
        if n > 0:
            u1 = (n - 1 + self.shift) // B
            f1 = min(u1, (n + B - 2) // B)
            rest = np.concatenate((self.fifo, np.zeros(B - self.fifo.shape[0], np.float32)))
            for u in range(n // B, u1 + 1):
                if u <= f1:
                    self._analyse(u, rest if u == n // B else np.zeros(B, np.float32))
                if u >= self.u0:
                    out.append(self._form(u, f1, n))
        self.reset()
        return np.concatenate(out) if out else np.zeros(0, np.float32)

    def run(self, x, cuts):
        """The concatenated output of x fed in `cuts`, flush included."""
        parts, at = [], 0
        for c in cuts:
            assert self.N == at
            parts.append(self.process(x[at:at + c]))
            assert parts[-1].shape[0] == emitted(at + c, self.shift) - emitted(at, self.shift)
            at += c
        assert at == x.shape[0]
        parts.append(self.flush())
        return np.concatenate(parts)


def causal_refs(x, h):
    """(ref32, ref64) of the CAUSAL alignment: y[m] = (x * g)[m], g = h reversed.  ref64 is numpy's float64 convolution; ref32 is
    convolve_reference.ref32 on the input delayed by k / 2 zeros, whose first n samples are the same sums."""
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    n, k = x.shape[0], h.shape[0]
    r64 = np.convolve(x.astype(np.float64), h[::-1].astype(np.float64))[:n]
    r32 = cr.ref32(np.concatenate((np.zeros(k // 2, np.float32), x)), h)[:n]
    return r32, r64
