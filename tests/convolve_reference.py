"""References, cases and the criterion of the long FIR convolution's tests (bsrnn_convolve_ragged), shared by tests/test_convolve_host.py
(CPU) and tests/test_gpu_convolve.py.  No test lives here.

ref64 is the definition: torch.nn.functional.conv1d(padding='same') in float64.  ref32 is the algorithm the kernels run (csrc/convolve_host.h:
uniformly partitioned overlap-save, B = 1024, partitions summed ascending) in float32 with torch.fft on the CPU - the float32 error the
criterion of tests/test_dsp_reference.py scales: e <= 3 * e_f32 + 2^-24 * max|ref64|, as max-abs per row and as L2 per block of 1024 samples.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from test_dsp_reference import hold

B = 1024
# (name, taps k, samples n): what each covers is in the table of tests/test_gpu_convolve.py
CASES = [("a", 1, 1), ("b", 1, 5000), ("c", 2, 5000), ("d", 1023, 3000), ("e", 1024, 3000), ("f", 1025, 3000), ("g", 2049, 5000),
         ("h", 3000, 500), ("i", 9300, 9221), ("j", 44101, 20000)]


def signal(n, seed):
    """0.1 * N(0, 1), float32, from the seed alone."""
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def decaying_noise(k, seed):
    """A synthetic room response: seeded noise under exp(-5 t / k), float32."""
    t = np.arange(k, dtype=np.float64)
    return (np.random.default_rng(seed).standard_normal(k) * np.exp(-5.0 * t / k)).astype(np.float32)


def ref64(x, h):
    """conv1d(x, h, padding='same') in float64: the definition."""
    xt = torch.from_numpy(np.asarray(x, np.float64)).reshape(1, 1, -1)
    ht = torch.from_numpy(np.asarray(h, np.float64)).reshape(1, 1, -1)
    return F.conv1d(xt, ht, padding="same").reshape(-1).numpy()


def plan(n, k):
    """Python restatement of conv_plan (csrc/convolve_host.h)."""
    P, shift = -(-k // B), k // 2
    u0, u1 = shift // B, (n - 1 + shift) // B
    last = (n + B - 2) // B
    return P, shift, u0, u1, max(0, u0 - (P - 1)), min(u1, last)


def ref32(x, h, drop=None):
    """The partitioned algorithm in float32 (complex64 spectra), partitions summed ascending.  drop = (block, partition): that block is
    computed without that partition (a wrong result the criterion must reject)."""
    x, h = np.asarray(x, np.float32), np.asarray(h, np.float32)
    n, k = x.shape[0], h.shape[0]
    P, shift, u0, u1, f0, f1 = plan(n, k)
    g = np.zeros(P * B, np.float32)
    g[:k] = h[::-1]
    part = np.zeros((P, 2 * B), np.float32)
    part[:, :B] = g.reshape(P, B)
    H = torch.fft.rfft(torch.from_numpy(part), dim=1)                       # complex64 [P, 1025]
    xp = np.zeros((u1 + 2) * B + B, np.float32)                             # x with B zeros in front: frame v = xp[v B : v B + 2 B]
    xp[B:B + n] = x
    frames = np.stack([xp[v * B:v * B + 2 * B] for v in range(u1 + 1)])
    X = torch.fft.rfft(torch.from_numpy(frames), dim=1)                     # [u1 + 1, 1025]
    Y = torch.zeros((u1 + 1, B + 1), dtype=torch.complex64)
    us = torch.arange(u0, u1 + 1)
    for p in range(P):                                                       # ascending; a frame outside [f0, f1] adds nothing
        v = us - p
        ok = (v >= f0) & (v <= f1)
        if drop is not None and p == drop[1]:
            ok &= us != drop[0]
        if ok.any():
            Y[us[ok]] += X[v[ok]] * H[p]
    y = torch.fft.irfft(Y[u0:], n=2 * B, dim=1)[:, B:].reshape(-1).numpy()   # blocks u0 .. u1 of x * g
    off = shift - u0 * B
    return y[off:off + n].astype(np.float32)


def block_with_last_partition(n, k):
    """(u, p): the last partition p any block's sum holds - P - 1 unless the filter is longer than the row, whose last partitions only meet
    frames past the row's end - and the middle one u of the blocks that hold it."""
    P, shift, u0, u1, f0, f1 = plan(n, k)
    for p in range(P - 1, -1, -1):
        us = [u for u in range(u0, u1 + 1) if f0 <= u - p <= f1]
        if us:
            return us[len(us) // 2], p


def hold_row(what, got, r32, r64):
    """The criterion on one row: max-abs over the row, L2 per block of 1024 output samples (the last block padded with zeros, which
    changes no norm)."""
    n = r64.shape[0]
    pad = -n % B
    a, b, c = (np.concatenate((np.asarray(v, np.float64), np.zeros(pad)))[None, :] for v in (got, r32, r64))
    return hold(what, a, b, c, per="hop")


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, h, ref32, ref64) of one case of the table, computed once per process and never written to."""
    i = [c[0] for c in CASES].index(name)
    _, k, n = CASES[i]
    x, h = signal(n, 100 + i), decaying_noise(k, 200 + i)
    out = (x, h, ref32(x, h), ref64(x, h))
    for a in out:
        a.setflags(write=False)
    return out
