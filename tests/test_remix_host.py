"""CPU-side tests of the re-mix (bsrnn_remix_ragged; augment.SourceShelf / remix_draw / remix_many; train.py --remix): the checks, the tile
count and the traffic model of csrc/remix_host.h against a brute-force restatement in Python (through tests/cpp/remix_plan_check.cpp,
built with -Wall -Werror and a second time with the address and undefined-behaviour sanitizers); declaration, export, binding and the
refusals on a host-only context; remix_draw against the reference's draw sequence written out on the global generator; train.py's new
arguments.  No compute here; tests/test_gpu_remix.py holds the kernel."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import remix_reference as rr
from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "remix_plan_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
TILE = 2048
MAX_LEN, MAX_EXTENT = 1 << 40, 1 << 60
(OK, NULL_TABLE, BAD_COUNT, BAD_WIDTH, MIX_STRIDE, TARGET_STRIDE, ROW_LENGTH, ROW_TERMS, TERM_LENGTH, TERM_OFFSET, TERM_SOURCE) = range(11)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output lines."""
    exe = str(tmp_path_factory.mktemp("remix") / "remix_plan_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["remix_host.h"]          # the host header only
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.split("\n")[:-1]
    return run


@pytest.fixture(scope="module")
def native():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    from speechseparation_amd import _native
    return _native


@pytest.fixture()
def host_ctx(native):
    from speechseparation_amd import spec
    v = spec.generate_bandsplits()[0]
    ctx = ctypes.c_void_p()
    assert native.lib.bsrnn_create(-1, (ctypes.c_int32 * len(v))(*v), len(v), ctypes.byref(ctx)) == 0
    yield ctx
    native.lib.bsrnn_destroy(ctx)


# ------------------------------------------------------------------------------------------------ remix_host.h
def brute(R, n_terms, mix_stride, target_stride, width, rows, terms, norows=False, noterms=False):
    """(why, index, tiles, read, written) from the header comment of include/bsrnn_hip.h alone: rows (n, first, count), terms
    (len, at, has_src); the traffic by counting samples one by one."""
    def stride_ok(s):
        return width <= s <= MAX_LEN and (R <= 1 or (R - 1) * s <= MAX_EXTENT)
    bad = (-1, -1, -1)
    if norows or noterms:
        return (NULL_TABLE, -1) + bad
    if R < 1 or n_terms < 1:
        return (BAD_COUNT, -1) + bad
    if not 0 <= width <= MAX_LEN:
        return (BAD_WIDTH, -1) + bad
    if not stride_ok(mix_stride):
        return (MIX_STRIDE, -1) + bad
    if not stride_ok(target_stride):
        return (TARGET_STRIDE, -1) + bad
    for r, (n, first, count) in enumerate(rows[:R]):
        if not 0 <= n <= width:
            return (ROW_LENGTH, r) + bad
        if count < 1 or first < 0 or first + count > n_terms:
            return (ROW_TERMS, r) + bad
    for t, (length, at, has_src) in enumerate(terms[:n_terms]):
        if not 0 <= length <= MAX_LEN:
            return (TERM_LENGTH, t) + bad
        if abs(at) > MAX_LEN:
            return (TERM_OFFSET, t) + bad
        if not has_src and length > 0:
            return (TERM_SOURCE, t) + bad
    reads = rr.reads_of([(n, [terms[t][:2] for t in range(first, first + count)]) for n, first, count in rows[:R]])
    return (OK, -1, -(-width // TILE), 4 * reads, 8 * width * R)


T5 = [(30, 0, 1), (10, -40, 1), (10, 25, 1), (100, -30, 1), (0, 7, 0)]      # inside; wholly left of a row of 20; wholly right; across; no samples, no source
CASES = {
    "n = 0": (1, 5, 20, 20, 20, [(0, 0, 5)], T5),
    "n = width": (1, 5, 20, 20, 20, [(20, 0, 5)], T5),
    "placements": (3, 5, 24, 21, 20, [(20, 0, 1), (20, 1, 3), (13, 3, 2)], T5),
    "rows share terms": (2, 5, 20, 20, 20, [(20, 0, 5), (7, 0, 5)], T5),
    "len = 0, null source": (1, 1, 5, 5, 5, [(5, 0, 1)], [(0, 0, 0)]),
    "term range out of the table": (2, 5, 20, 20, 20, [(20, 0, 5), (20, 3, 3)], T5),
    "term range, negative first": (1, 5, 20, 20, 20, [(20, -1, 2)], T5),
    "row without terms": (1, 5, 20, 20, 20, [(20, 0, 0)], T5),
    "width > mix_stride": (1, 5, 19, 20, 20, [(20, 0, 5)], T5),
    "width > target_stride": (1, 5, 20, 19, 20, [(20, 0, 5)], T5),
    "n > width": (2, 5, 20, 20, 20, [(20, 0, 5), (21, 0, 5)], T5),
    "n < 0": (1, 5, 20, 20, 20, [(-1, 0, 5)], T5),
    "null source with samples": (1, 2, 20, 20, 20, [(20, 0, 2)], [(3, 0, 1), (3, 0, 0)]),
    "len < 0": (1, 1, 20, 20, 20, [(20, 0, 1)], [(-1, 0, 1)]),
    "at beyond the bound": (1, 1, 20, 20, 20, [(20, 0, 1)], [(1, MAX_LEN + 1, 1)]),
    "R = 0": (0, 5, 20, 20, 20, [(20, 0, 5)], T5),
    "n_terms = 0": (1, 0, 20, 20, 20, [(20, 0, 5)], T5),
    "width < 0": (1, 5, 20, 20, -1, [(0, 0, 5)], T5),
    "width = 0": (1, 5, 0, 0, 0, [(0, 0, 5)], T5),
    "stride beyond 2^40": (1, 5, (1 << 40) + 1, 20, 20, [(20, 0, 5)], T5),
    "several tiles": (2, 5, 3 * TILE + 8, 3 * TILE + 5, 3 * TILE + 5, [(3 * TILE + 5, 0, 5), (TILE + 1, 0, 2)], [(5000, -100, 1), (9000, 4000, 1)] + T5[2:]),
}


def _argv(case, extra=()):
    R, n_terms, ms, ts, width, rows, terms = case
    return ["check", R, n_terms, ms, ts, width, *extra, *["r:%d:%d:%d" % r for r in rows], *["t:%d:%d:%d" % t for t in terms]]


@pytest.mark.parametrize("name", list(CASES))
def test_verdict_tiles_and_traffic_against_brute_force(check, name):
    case = CASES[name]
    want = brute(*case)
    assert check(*_argv(case)) == ["%d %d %d %d %d" % want], (name, want)
    if name in ("n = 0", "n = width", "placements", "rows share terms", "len = 0, null source", "width = 0", "several tiles"):
        assert want[0] == OK, name
    else:
        assert want[0] != OK, name


def test_null_tables_and_tile_edges(check):
    case = CASES["n = width"]
    assert check(*_argv(case, ["norows"])) == ["%d -1 -1 -1 -1" % NULL_TABLE]
    assert check(*_argv(case, ["noterms"])) == ["%d -1 -1 -1 -1" % NULL_TABLE]
    for width in (1, TILE - 1, TILE, TILE + 1, 2205000):
        line = check("check", 1, 1, width, width, width, "r:%d:0:1" % width, "t:%d:0:1" % width)[0].split()
        assert [int(v) for v in line] == [OK, -1, -(-width // TILE), 4 * width, 8 * width]


def test_self_checks_under_the_sanitizers(check, tmp_path):
    assert check("self") == ["ok"]
    assert check("limits") == ["256 8 %d %d %d 32 16" % (TILE, MAX_LEN, MAX_EXTENT)]
    exe = str(tmp_path / "remix_plan_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    for args in (["self"], _argv(CASES["placements"]), _argv(CASES["term range out of the table"]), _argv(CASES["several tiles"]),
                 _argv(CASES["n = width"], ["norows"])):
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == 0 and out.stdout.strip(), out.stdout + out.stderr


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_symbol():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+bsrnn_remix_ragged\s*\(([^)]*)\)\s*;", body, flags=re.M)
    assert m and m.group(1).strip() == "int"
    got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
    assert got == ["bsrnn_ctx*", "constbsrnn_remix_row*", "int32_t", "constbsrnn_remix_term*", "int32_t", "float*", "int64_t", "float*", "int64_t",
                   "int64_t", "void*"]
    assert re.search(r"typedef struct bsrnn_remix_term \{ const float\* src; int64_t len; int64_t at; float gain; int32_t pad_; \} bsrnn_remix_term;", body)
    assert re.search(r"typedef struct bsrnn_remix_row\s+\{ int64_t n; int32_t first_term; int32_t n_terms; \} bsrnn_remix_row;", body)
    assert re.search(r"#define\s+BSRNN_REMIX_TILE\s+%d\b" % TILE, body)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body)
    assert "m_dataset.py:141-180" in txt and "UNDEFINED" in txt          # overlapping outputs and sources: said, not checked


def test_symbol_is_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    assert "bsrnn_remix_ragged" in native.SYMBOLS and "bsrnn_remix_ragged" in exported
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_remix_ragged.argtypes == [vp, ctypes.POINTER(native.RemixRowC), i32, ctypes.POINTER(native.RemixTermC), i32, vp, i64, vp,
                                                      i64, i64, vp]
    assert ctypes.sizeof(native.RemixTermC) == 32 and ctypes.sizeof(native.RemixRowC) == 16
    assert (native.RemixTermC.src.offset, native.RemixTermC.len.offset, native.RemixTermC.at.offset, native.RemixTermC.gain.offset) == (0, 8, 16, 24)
    assert (native.RemixRowC.n.offset, native.RemixRowC.first_term.offset, native.RemixRowC.n_terms.offset) == (0, 8, 12)
    assert native.REMIX_TILE == TILE
    assert native.lib.bsrnn_abi_version() == 2


def test_argument_errors_without_a_device(native, host_ctx):
    lib = native.lib

    def err():
        return lib.bsrnn_last_error().decode()
    import numpy as np
    src, a, b = np.ones(8, np.float32), np.zeros((2, 12), np.float32), np.zeros((2, 12), np.float32)
    pa, pb = a.ctypes.data_as(ctypes.c_void_p), b.ctypes.data_as(ctypes.c_void_p)
    rows = (native.RemixRowC * 2)((10, 0, 2), (0, 2, 1))
    terms = (native.RemixTermC * 3)((src.ctypes.data, 8, -1, 1.0, 0), (src.ctypes.data, 8, 5, 0.5, 0), (None, 0, 0, 1.0, 0))
    call = lib.bsrnn_remix_ragged
    assert call(None, rows, 2, terms, 3, pa, 12, pb, 12, 10, None) == EARG and "null context" in err()
    assert call(host_ctx, None, 2, terms, 3, pa, 12, pb, 12, 10, None) == EARG and "rows_host" in err(), err()
    assert call(host_ctx, rows, 2, None, 3, pa, 12, pb, 12, 10, None) == EARG and "terms_host" in err(), err()
    assert call(host_ctx, rows, 2, terms, 3, None, 12, pb, 12, 10, None) == EARG and "mix_dev" in err(), err()
    assert call(host_ctx, rows, 2, terms, 3, pa, 12, None, 12, 10, None) == EARG and "target_dev" in err(), err()
    for R in (0, -1):
        assert call(host_ctx, rows, R, terms, 3, pa, 12, pb, 12, 10, None) == EARG and "R = %d" % R in err(), err()
    assert call(host_ctx, rows, 2, terms, 0, pa, 12, pb, 12, 10, None) == EARG and "n_terms = 0" in err(), err()
    assert call(host_ctx, rows, 2, terms, 3, pa, 12, pb, 12, -1, None) == EARG and "width = -1" in err(), err()
    assert call(host_ctx, rows, 2, terms, 3, pa, 9, pb, 12, 10, None) == EARG and "mix_stride 9" in err(), err()
    assert call(host_ctx, rows, 2, terms, 3, pa, 12, pb, 9, 10, None) == EARG and "target_stride 9" in err(), err()
    assert call(host_ctx, rows, 2, terms, 3, pa, 12, pb, 12, 9, None) == EARG and "rows_host[0].n = 10" in err(), err()
    assert call(host_ctx, rows, 2, terms, 2, pa, 12, pb, 12, 10, None) == EARG and "rows_host[1]" in err() and "[0, 2)" in err(), err()
    bad = (native.RemixTermC * 3)((src.ctypes.data, 8, -1, 1.0, 0), (None, 8, 5, 0.5, 0), (None, 0, 0, 1.0, 0))
    assert call(host_ctx, rows, 2, bad, 3, pa, 12, pb, 12, 10, None) == EARG and "terms_host[1].src is null" in err(), err()
    bad = (native.RemixTermC * 3)((src.ctypes.data, -8, -1, 1.0, 0), (src.ctypes.data, 8, 5, 0.5, 0), (None, 0, 0, 1.0, 0))
    assert call(host_ctx, rows, 2, bad, 3, pa, 12, pb, 12, 10, None) == EARG and "terms_host[0].len = -8" in err(), err()
    # valid arguments: a host-only context cannot compute, and nothing was touched
    assert call(host_ctx, rows, 2, terms, 3, pa, 12, pb, 12, 10, None) == ESTATE and "host-only" in err(), err()
    assert not a.any() and not b.any()


# ------------------------------------------------------------------------------------------------ the draws
class FakeShelf:
    """Sources as lengths only: what remix_draw asks of a shelf."""

    def __init__(self, dialogs, backgrounds):
        self.lengths = {"dialog": list(dialogs), "background": list(backgrounds)}
        self.n_dialogs, self.n_backgrounds = len(dialogs), len(backgrounds)

    def length_of(self, kind, i):
        return self.lengths[kind][i]


def test_remix_draw_makes_the_reference_draws(native):
    from speechseparation_amd import augment
    length = 5000
    dialogs = [3000, 12000, 4999, 5001, 700, 90000, 5002]
    backgrounds = [100, 5001, 4999, 20000, 7000, 2500, 5003, 60000, 1, 9999, 4000]
    shelf = FakeShelf(dialogs, backgrounds)
    state = random.getstate()
    try:
        seen_pad = seen_cut = 0
        for idx in range(200):
            dialog, chosen, at, gains, scale = rr.reference_draws(idx, dialogs, backgrounds, length)
            sp = augment.remix_draw(idx, shelf, length)
            assert (sp.dialog, list(sp.backgrounds), list(sp.at), sp.length) == (dialog, chosen, at, length), idx
            assert list(sp.gain) == [1.0] + gains, idx                       # the reference's dialog scale is drawn and not applied
            sp2 = augment.remix_draw(idx, shelf, length, scale_dialog=True)
            assert list(sp2.gain) == [scale] + gains and sp2[:3] == sp[:3], idx
            seen_pad += sum(a > 0 for a in at)
            seen_cut += sum(a < 0 for a in at)
        assert seen_pad > 100 and seen_cut > 100                             # shorter and longer sources both occurred
        dialog, chosen, at, gains, scale = rr.reference_draws(7, dialogs, backgrounds, length, n_backgrounds=2)
        sp = augment.remix_draw(7, shelf, length, n_backgrounds=2)
        assert (sp.dialog, list(sp.backgrounds), list(sp.at), list(sp.gain)) == (dialog, chosen, at, [1.0] + gains)
    finally:
        random.setstate(state)
    assert list(__import__("inspect").signature(augment.remix_draw).parameters) == ["idx", "shelf", "length", "n_backgrounds", "scale_dialog"]
    d = __import__("inspect").signature(augment.remix_draw).parameters
    assert (d["length"].default, d["n_backgrounds"].default, d["scale_dialog"].default) == (50 * 44100, 4, False)


def test_a_source_of_exactly_the_length_raises(native):
    from speechseparation_amd import augment
    with pytest.raises(ValueError):
        augment.remix_draw(0, FakeShelf([5000], [100, 7000]), 5000)
    with pytest.raises(ValueError):
        augment.remix_draw(0, FakeShelf([300], [5000]), 5000)
    augment.remix_draw(0, FakeShelf([4999], [5001]), 5000)


def test_python_layer_signatures(native):
    import inspect
    from speechseparation_amd import augment, train
    assert list(inspect.signature(augment.SourceShelf.__init__).parameters) == ["self", "device"]
    for name in ("add_dialog", "add_background", "add_sections", "length_of", "__len__"):
        assert callable(getattr(augment.SourceShelf, name)), name
    assert isinstance(augment.SourceShelf.n_dialogs, property) and isinstance(augment.SourceShelf.n_backgrounds, property)
    sig = inspect.signature(augment.remix_many)
    assert list(sig.parameters) == ["shelf", "specs", "length", "out"] and sig.parameters["out"].default is None
    sig = inspect.signature(train.train_step_packed)
    assert list(sig.parameters) == ["model", "optimizer", "mix", "speech", "lengths", "clip_rows", "group", "loss_sdr"]
    assert sig.parameters["group"].default is None and sig.parameters["loss_sdr"].default is False
    with pytest.raises(ValueError):
        augment.SourceShelf("cpu")


# ------------------------------------------------------------------------------------------------ train.py --remix
@pytest.fixture(scope="module")
def entry(native):
    import importlib.util
    spec_ = importlib.util.spec_from_file_location("train_entry_remix", os.path.join(REPO, "train.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    return mod


PARENT_DEFAULTS = {'datapath': None, 'mini': False, 'batch_size': 1, 'resume': False, 'train_folder': None, 'val_folder': 'val', 'loss_sdr': False,
                   'epochs': 1, 'synthetic': 2, 'seconds': 4.0, 'synthetic_weights': None, 'graph': False, 'ragged': False, 'device': None,
                   'outdir': '.', 'rir': None, 'rir_prob': 0.1, 'rir_rate': 16000}      # what the parser gave for --synthetic 2 before --remix


def test_train_arguments(entry, capsys):
    ap = entry.build_parser()
    args = entry.parse_args(ap, ["--remix", "/somewhere", "--batch_size", "3"])
    assert (args.remix, args.remix_seconds, args.remix_backgrounds, args.batch_size) == ("/somewhere", 50.0, 4, 3)
    args = entry.parse_args(ap, ["--remix", "d", "--remix_seconds", "2.5", "--remix_backgrounds", "2"])
    assert (args.remix_seconds, args.remix_backgrounds) == (2.5, 2)
    got = vars(entry.parse_args(ap, ["--synthetic", "2"]))
    new = {"remix": None, "remix_seconds": 50.0, "remix_backgrounds": 4}
    assert got == {**PARENT_DEFAULTS, **new}
    for extra in (["--rir", "rirs"], ["--graph"]):
        with pytest.raises(SystemExit) as e:
            entry.main(["--remix", "d"] + extra)
        assert e.value.code == 2
        assert "--remix does not go with --rir or --graph" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        entry.parse_args(ap, ["--remix", "d", "--remix_seconds", "0.01"])


def test_remix_file_listing(entry, tmp_path):
    names = ["a/speech.wav", "a/sfx.wav", "a/music.wav", "a/mixture.wav", "b/speech_post_rnnoise.wav", "b/vocalnoise_3.wav", "b/vocalnoise.txt",
             "c/lownoise_take.wav", "c/lownoise/anything.wav", "c/speech.flac", "c/sfx_bg.flac", "mined/dialog-2048.wav", "mined/background-9216.wav",
             "mined/dialog-1.txt", "mined/sfx.wav.bak"]
    for n in names:
        p = tmp_path / n
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
    dialogs, backgrounds, flac = entry.remix_files(str(tmp_path))
    rel = lambda ps: [os.path.relpath(p, str(tmp_path)) for p in ps]          # noqa: E731
    assert rel(dialogs) == ["a/speech.wav", "b/speech_post_rnnoise.wav", "c/lownoise_take.wav", "c/lownoise/anything.wav", "mined/dialog-2048.wav"]
    assert rel(backgrounds) == ["a/music.wav", "a/sfx.wav", "b/vocalnoise_3.wav", "mined/background-9216.wav"]
    assert flac == 2
