"""GPU: the long FIR convolution of ragged rows (augment.FirBank -> bsrnn_fir_bank_*, bsrnn_convolve_ragged).

The definition is torch.nn.functional.conv1d(padding='same') in float64 (convolve_reference.ref64); the bound is the project's DSP criterion
(tests/test_dsp_reference.py): e <= 3 * e_f32 + 2^-24 * max|ref64|, as max-abs per row and as L2 per block of 1024 output samples, with
e_f32 the error of the same partitioned algorithm in float32 with torch.fft on the CPU (convolve_reference.ref32) - never the kernel's own.

    case   k       n       what it covers
    a      1       1       smallest sizes
    b      1       5000    single tap
    c      2       5000    even taps
    d      1023    3000    one partition, just under a block
    e      1024    3000    exactly one block
    f      1025    3000    two partitions, odd shift
    g      2049    5000    three partitions
    h      3000    500     filter longer than the row
    i      9300    9221    more partitions than a tile, more blocks than a tile
    j      44101   20000   a real RIR length

(The multiply-accumulate ships with a tile of 16 blocks: case i is a partial tile with a partial pass over the partitions, case j - 44
partitions, 21 blocks - has more of both than a tile, and the row-group test 977 blocks per row.)

All ten rows go through ONE call - every row its own length and filter, rows n_max + 3 floats apart.  The only comparisons of the library
with itself are the equalities the interface promises (a row in a batch == the row alone, a view == its contiguous copy, a row of a
grouped call == the row alone, a copied row == the input)."""
import ctypes

import numpy as np
import pytest
import torch

import convolve_reference as cr

pytestmark = pytest.mark.gpu
EARG = 1
NAMES = [c[0] for c in cr.CASES]
SENTINEL = 777.0


@pytest.fixture(scope="module")
def model(sd_default):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in sd_default.items()}, strict=True)
    return m.to("cuda")


@pytest.fixture(scope="module")
def bank(model):
    """One filter per case, in the table's order."""
    from speechseparation_amd.augment import FirBank
    return FirBank(model, [cr.case(name)[1] for name in NAMES])


@pytest.fixture(scope="module")
def batch(bank):
    """The ten cases as the rows of one call: (input buffer, its copy from before the call, output buffer, lengths).  Rows are n_max + 3
    floats apart in both buffers; the output starts as a sentinel."""
    lens = [c[2] for c in cr.CASES]
    n_max = max(lens)
    buf = torch.zeros((len(lens), n_max + 3), device="cuda")
    for r, name in enumerate(NAMES):
        buf[r, :lens[r]] = torch.from_numpy(cr.case(name)[0].copy())
        buf[r, lens[r]:] = 5.0                                   # what lies behind a row must not be read
    before = buf.clone()
    out = torch.full((len(lens), n_max + 3), SENTINEL, device="cuda")
    res = bank.convolve(buf[:, :n_max], lens, list(range(len(lens))), out=out[:, :n_max])
    assert res.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return buf, before, out, lens


def test_bank_reports_its_filters(bank):
    assert len(bank) == len(NAMES) and [bank.taps(i) for i in range(len(bank))] == [c[1] for c in cr.CASES]
    with pytest.raises(IndexError):
        bank.taps(len(bank))


@pytest.mark.parametrize("name", NAMES)
def test_parity(batch, name):
    buf, before, out, lens = batch
    r = NAMES.index(name)
    x, h, r32, r64 = cr.case(name)
    got = out[r, :lens[r]].cpu().numpy()
    cr.hold_row("case %s (k = %d, n = %d)" % (name, h.shape[0], x.shape[0]), got, r32, r64)


def test_the_call_touches_nothing_else(batch):
    buf, before, out, lens = batch
    assert torch.equal(buf, before)                              # the input is unchanged
    for r, n in enumerate(lens):
        assert bool((out[r, n:] == SENTINEL).all()), r           # samples past lens[r], the 3 floats between rows included


def test_every_row_equals_the_row_alone(bank, batch):
    """Mixed batch (copied rows among them) against R = 1 calls of contiguous rows: bit for bit."""
    buf, before, out, lens = batch
    n_max = max(lens)
    filt = [r if r % 4 != 1 else -1 for r in range(len(lens))]
    mixed = bank.convolve(buf[:, :n_max], lens, filt)
    for r, n in enumerate(lens):
        alone = bank.convolve(buf[r:r + 1, :n].contiguous(), [n], [filt[r]])
        assert torch.equal(mixed[r, :n], alone[0]), r
        assert not mixed[r, n:].any()
        if filt[r] < 0:
            assert torch.equal(mixed[r, :n], buf[r, :n])         # filter -1: the input, exactly
        else:
            assert torch.equal(mixed[r, :n], out[r, :n])         # and the bits of the ten-row call


def test_views_equal_their_copies(bank):
    """A channel slice of a [clips, 2, n] buffer (row stride 2 n) and a column slice at an odd float, into an output view at an odd float."""
    g = torch.Generator().manual_seed(5)
    clips = (0.1 * torch.randn((3, 2, 6000), generator=g)).cuda()
    lens, filt = [6000, 4097, 1], [6, 5, 8]
    ref = bank.convolve(clips[:, 1].contiguous(), lens, filt)
    assert torch.equal(bank.convolve(clips[:, 1], lens, filt), ref)
    wide = torch.zeros((3, 6011), device="cuda")
    wide[:, 7:6007] = clips[:, 1]
    out = torch.full((3, 6011), SENTINEL, device="cuda")
    bank.convolve(wide[:, 7:6007], lens, filt, out=out[:, 3:6003])
    for r, n in enumerate(lens):
        assert torch.equal(out[r, 3:3 + n], ref[r, :n]), r
        assert bool((out[r, :3] == SENTINEL).all()) and bool((out[r, 3 + n:] == SENTINEL).all())


def test_row_groups(model):
    """70 rows of 1 000 000 samples under 3 taps need 70 * 978 input frames: more than the budget of 65 536, so the call runs as two row
    groups.  Rows 0 and 69 equal their single-row calls bit for bit; every row meets the criterion against the float64 shifted add."""
    from speechseparation_amd.augment import FirBank
    R, n = 70, 1000000
    h = np.array([0.25, 0.5, -0.125], np.float32)
    bank3 = FirBank(model, [h])
    g = torch.Generator().manual_seed(9)
    x = 0.1 * torch.randn((R, n), generator=g)
    xd = x.cuda()
    y = bank3.convolve(xd)
    for r in (0, R - 1):
        assert torch.equal(bank3.convolve(xd[r:r + 1])[0], y[r]), r
    got = y.cpu().numpy()
    x64 = np.zeros((R, n + 2))
    x64[:, 1:-1] = x.numpy()
    r64 = float(h[0]) * x64[:, :-2] + float(h[1]) * x64[:, 1:-1] + float(h[2]) * x64[:, 2:]      # left = 1
    for r in range(R):
        cr.hold_row("row group row %d" % r, got[r], cr.ref32(x[r].numpy(), h), r64[r])


def test_refusals_and_the_next_call(bank, batch):
    """Every refusal returns BSRNN_EARG with its sentence, and the next valid call succeeds."""
    from speechseparation_amd import _native
    lib = _native.lib
    buf, before, out, lens = batch
    a = torch.zeros((2, 100), device="cuda")
    b = torch.zeros((2, 100), device="cuda")
    pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
    i64s, i32s = (lambda *v: (ctypes.c_int64 * len(v))(*v)), (lambda *v: (ctypes.c_int32 * len(v))(*v))
    good = (bank._h, pa, 100, i64s(100, 40), i32s(0, -1), pb, 100, 2, None)

    def refused(sentence, **change):
        names = ["bank", "in", "in_stride", "lens", "filt", "out", "out_stride", "R", "stream"]
        args = [change.get(k, v) for k, v in zip(names, good)]
        assert lib.bsrnn_convolve_ragged(*args) == EARG, sentence
        assert sentence in lib.bsrnn_last_error().decode(), lib.bsrnn_last_error().decode()
        assert lib.bsrnn_convolve_ragged(*good) == 0                     # the next valid call
    refused("null FIR bank", bank=None)
    for k in ("in", "lens", "filt", "out"):
        refused("null argument", **{k: None})
    refused("R = 0", R=0)
    refused("lens_host[1] = 0", lens=i64s(100, 0))
    refused("in_stride 99", in_stride=99)
    refused("out_stride 50", out_stride=50)
    refused("filter_host[0] = %d" % len(bank), filt=i32s(len(bank), -1))
    refused("filter_host[1] = -2", filt=i32s(0, -2))
    refused("overlap", out=pa)
    refused("overlap", out=ctypes.c_void_p(a.data_ptr() + 4 * 139))          # the last sample the rows span
    torch.cuda.synchronize()
    with pytest.raises(_native.NativeError):
        bank.convolve(torch.zeros((2, 100)))                                  # a CPU tensor
    if torch.cuda.device_count() > 1:                                         # a bank of another context's device
        other = torch.zeros((2, 100), device="cuda:1")
        with pytest.raises(ValueError):
            bank.convolve(other)
        refused("lies on device", **{"in": ctypes.c_void_p(other.data_ptr())})
    # and the results are still those of the first call
    n_max = max(lens)
    again = bank.convolve(buf[:, :n_max], lens, list(range(len(lens))))
    for r, n in enumerate(lens):
        assert torch.equal(again[r, :n], out[r, :n])
