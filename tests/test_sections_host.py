"""CPU-side tests of the section mining (bsrnn_hop_activity, bsrnn_section_*, bsrnn_sections_scan): the run-length state machine of
csrc/sections_host.h against the numpy restatement of tests/sections_reference.py (through tests/cpp/sections_check.cpp, built with
-Wall -Werror and a second time with the address and undefined-behaviour sanitizers) on seeded sequences from a palette that reaches
every branch, on the rule's edges, in every split; declarations, exports, bindings and the refusals on a host-only context.  No compute
here; tests/test_gpu_activity.py holds the kernel, tests/test_gpu_mining.py the device path."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import sections_reference as sr
from conftest import REPO

LIB = os.path.join(REPO, "speechseparation_amd", "lib", "libbsrnn_hip.so")
CSRC = os.path.join(REPO, "speechseparation_amd", "csrc")
SRC = os.path.join(REPO, "tests", "cpp", "sections_check.cpp")
EARG, ESTATE = 1, 2          # BSRNN_EARG, BSRNN_ESTATE of include/bsrnn_hip.h
NEW = ["bsrnn_hop_activity", "bsrnn_section_rule_default", "bsrnn_section_state_reset", "bsrnn_sections_scan"]
INF, NAN = math.inf, math.nan

# (ratio, level mean) literals.  10 ln(ratio): 7.5 -> 20.1, 2.0 -> 6.9, 1.0 -> 0, 0.1 -> -23.0, 0.01 -> -46.1;
# 10 ln(level mean): 1e-2 -> -46 (above -100), 1e-5 -> -115 (below), 1.01e-10 -> -230 (just over the floor), 0.99e-10 -> the floor's -200
LOUD, QUIET, OVER, UNDER = 1e-2, 1e-5, 1.01e-10, 0.99e-10
PALETTE = [(7.5, LOUD), (7.5, QUIET), (2.0, LOUD), (2.0, QUIET), (1.0, LOUD), (0.1, LOUD), (1.0, QUIET), (0.01, LOUD), (0.01, QUIET),
           (INF, LOUD), (INF, QUIET), (0.0, LOUD), (0.0, QUIET), (NAN, LOUD), (NAN, QUIET), (1.0, OVER), (1.0, UNDER), (NAN, OVER), (NAN, UNDER)]
D, BR, N, G, S = (7.5, LOUD), (2.0, LOUD), (1.0, LOUD), (0.01, LOUD), (NAN, QUIET)      # dialog, bridge, neither, background, silent
RULES = [{}, {"min_run": 1}, {"silence_db": -210.0, "min_run": 3}]


def rule_args(rule):
    q = dict(sr.DEFAULT_RULE, **rule)
    return [repr(float(q[k])) for k in ("dialog_db", "bridge_db", "background_db", "silence_db", "level_floor", "floor_db")] + [str(q["min_run"])]


def sequence(seed, n=300):
    """Runs of palette entries, of lengths around min_run, so that sections open, bridge, change kind and reset."""
    rng = np.random.RandomState(seed)
    hops = []
    while len(hops) < n:
        hops += [PALETTE[rng.randint(len(PALETTE))]] * int(rng.choice([1, 1, 2, 3, 9, 10, 11, 15]))
    return np.array(hops[:n], np.float64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """The stand-alone program, built as its neighbours are (g++ -Wall -Werror); run(*args) gives its output lines."""
    d = tmp_path_factory.mktemp("sections")
    exe = str(d / "sections_check")
    assert re.findall(r'#include\s+"([^"]+)"', open(SRC).read()) == ["sections_host.h"]          # the host header only
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe], check=True)
    count = [0]

    def run(*args, act=None, exe=exe, ok=0):
        args = list(args)
        if act is not None:
            count[0] += 1
            path = str(d / ("act%d.f64" % count[0]))
            np.ascontiguousarray(act, np.float64).tofile(path)
            args.insert(1, path)
        out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert out.returncode == ok, out.stdout + out.stderr
        return out.stdout.split("\n")[:-1]
    return run


def scan(check, act, rule=None, cap=None, flush=True, splits=(), **kw):
    """-> (sections written per feed, n_out per feed, final state)"""
    act = np.asarray(act, np.float64).reshape(-1, 2)
    cap = len(act) + 1 if cap is None else cap
    lines = check("scan", *(rule_args(rule or {}) + [cap, int(flush)] + list(splits)), act=act, **kw)
    feeds, counts = [], []
    for ln in lines[:-1]:
        if ln.startswith("feed"):
            feeds.append([])
            counts.append(int(ln.split()[1]))
        else:
            feeds[-1].append(tuple(int(v) for v in ln.split()))
    assert lines[-1].startswith("state")
    return feeds, counts, tuple(int(v) for v in lines[-1].split()[1:])


def native_state(s):
    return (s.n_dialog, s.n_background, 0 if s.open is None else s.open[0], 0 if s.open is None else s.open[1], s.hop)


# ------------------------------------------------------------------------------------------------ sections_host.h
def test_palette_is_clear_of_the_thresholds_and_reaches_every_class(check):
    """The precondition of every comparison below (`check`: the palette is for the header's scanner, there is nothing to hold without it)."""
    for rule in RULES:
        assert sr.clear_of_thresholds(np.array(PALETTE), margin=1e-6, **rule)
    q = sr.DEFAULT_RULE
    dbs = [sr.to_db(r) for r, _ in PALETTE]
    assert any(d > q["dialog_db"] and d < INF for d in dbs) and any(q["bridge_db"] < d <= q["dialog_db"] for d in dbs)
    assert any(q["background_db"] <= d <= q["bridge_db"] for d in dbs) and any(-INF < d < q["background_db"] for d in dbs)
    for special in (lambda d: d == INF, lambda d: d == -INF, math.isnan):
        levels = [sr.to_level(lv, q) for (r, lv), d in zip(PALETTE, dbs) if special(d)]
        assert any(v < q["silence_db"] for v in levels) and any(v > q["silence_db"] for v in levels)
    assert sr.to_level(UNDER, q) == q["floor_db"] and abs(sr.to_level(OVER, q) - 10 * math.log(OVER)) < 1e-9
    assert abs(UNDER - q["level_floor"]) < 2e-12 and abs(OVER - q["level_floor"]) < 2e-12


def test_defaults_and_refusals_of_the_header(check):
    assert check("defaults") == ["10 3 -30 -100 1e-10 -200 10 | 0 0 0 0 0"]
    # null state, null count, negative hops, negative cap, min_run 0, null activity with hops; then two valid sets
    assert check("refusals") == ["1 2 3 3 4 5 0 0"]


@pytest.mark.parametrize("rule", RULES, ids=["default", "min_run_1", "silence_210_min_run_3"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_scanner_against_the_restatement(check, seed, rule):
    act = sequence(seed)
    want = sr.scan(act, **rule)
    feeds, counts, state = scan(check, act, rule)
    assert feeds == [want] and counts == [len(want)]
    if not rule:
        assert {k for k, a, b in want} == {sr.DIALOG, sr.BACKGROUND}, "the sequence closes sections of both kinds"
    # without a flush the state is the restatement's
    ref = sr.Scanner(**rule)
    want_open = ref.feed(act)
    feeds, counts, state = scan(check, act, rule, flush=False)
    assert feeds == [want_open] and state == native_state(ref)
    assert check("splits", *rule_args(rule), act=act) == ["ok %d" % len(want)]


def test_every_branch_follows_every_branch(check):
    """On the restatement: with the default rule the seeded sequences that the header's scanner is compared on take the four branches in
    every order that exists."""
    seen = set()
    for seed in (1, 2, 3):
        ref, prev = sr.Scanner(), None
        for ratio, lv in sequence(seed):
            db, level = sr.to_db(float(ratio)), sr.to_level(float(lv), ref.rule)
            if db > 10:
                br = 1
            elif (db > 3 or level < -100) and ref.n_dialog >= 10:
                br = 2
            elif db < -30:
                br = 3
            else:
                br = 4
            ref.feed([[ratio, lv]])
            seen.add((prev, br))
            prev = br
    # (branches 3 and 4 leave n_dialog at 0, so a bridge cannot follow them: fourteen orders exist)
    assert {(a, b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4)} - {(3, 2), (4, 2)} == seen - {(None, b) for b in (1, 2, 3, 4)}


def test_edges_of_the_rule(check):
    def both(hops, rule=None, **kw):
        want = sr.scan(hops, **(rule or {})) if kw.get("flush", True) else sr.Scanner(**(rule or {})).feed(hops)
        feeds, counts, state = scan(check, hops, rule, **kw)
        assert feeds == [want], (feeds, want)
        return want, state
    # runs of min_run - 1, min_run, min_run + 1: the section opens AT the min_run-th hop
    assert both([D] * 9 + [N] * 3)[0] == []
    assert both([D] * 10 + [N] * 3)[0] == [(1, 9, 10)]
    assert both([D] * 11 + [N] * 3)[0] == [(1, 9, 11)]
    assert both([G] * 9 + [N])[0] == [] and both([G] * 10 + [N])[0] == [(2, 9, 10)] and both([G] * 11 + [N])[0] == [(2, 9, 11)]
    # a bridge hop with n_dialog = min_run - 1 resets: the five dialog hops behind it do not complete a run
    assert both([D] * 9 + [BR] + [D] * 5)[0] == [] and both([D] * 9 + [S] + [D] * 5)[0] == []
    # with n_dialog = min_run it bridges, by db or by silence (a NaN db included), and the counters stay
    assert both([D] * 10 + [BR, S, BR] + [D] + [N])[0] == [(1, 9, 14)]
    # dialog -> background directly: the first background hop closes the dialog section, the tenth opens a background section
    assert both([D] * 12 + [G] * 12)[0] == [(1, 9, 12), (2, 21, 24)]
    assert both([G] * 12 + [D] * 12)[0] == [(2, 9, 12), (1, 21, 24)]
    # a ratio of exactly 0 is -inf dB: background; +inf is dialog
    assert both([(0.0, LOUD)] * 10 + [(INF, LOUD)] * 10)[0] == [(2, 9, 10), (1, 19, 20)]
    # a flush with a section open and with none; no flush leaves it open in the state
    assert both([D] * 12)[0] == [(1, 9, 12)]
    assert both([D] * 12, flush=False) == ([], (12, 0, 1, 9, 12))
    assert both([N] * 4)[0] == [] and both([])[0] == []
    # cap smaller than the count: the first `cap` are written, the count is whole, the state has advanced over everything
    hops = ([D] * 11 + [N]) * 3
    want = sr.scan(hops)
    assert len(want) == 3
    for cap in (0, 1, 2, 3):
        feeds, counts, state = scan(check, hops, cap=cap)
        assert feeds == [want[:cap]] and counts == [3] and state == (0, 0, 0, 0, 36)
    # a non-default rule: min_run = 1 opens at the first hop
    assert both([D, N, G, G, D], {"min_run": 1})[0] == [(1, 0, 1), (2, 2, 4), (1, 4, 5)]
    # the level floor: just under it the level is floor_db, just over it 10 ln(level) - told apart by a silence threshold between them
    r = {"silence_db": -210.0, "min_run": 1}
    assert both([D, (1.0, OVER), N], r)[0] == [(1, 0, 2)] and both([D, (1.0, UNDER), N], r)[0] == [(1, 0, 1)]


def test_splits_and_hop_by_hop(check):
    act = sequence(7, 120)
    want = sr.scan(act)
    assert want
    assert check("splits", *rule_args({}), act=act) == ["ok %d" % len(want)]
    feeds, counts, state = scan(check, act, splits=["each"])
    assert [s for f in feeds for s in f] == want and len(feeds) == 120
    feeds, counts, state = scan(check, act, splits=[0, 13, 13, 60])
    assert [s for f in feeds for s in f] == want and len(feeds) == 5


def test_under_the_sanitizers(check, tmp_path):
    exe = str(tmp_path / "sections_check_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, SRC, "-o", exe], check=True)
    assert check("defaults", exe=exe) and check("refusals", exe=exe) == ["1 2 3 3 4 5 0 0"]
    act = sequence(5)
    want = sr.scan(act)
    assert scan(check, act, exe=exe)[0] == [want]
    assert scan(check, act, cap=1, exe=exe)[0] == [want[:1]]               # out holds exactly cap sections
    assert scan(check, act, cap=0, splits=["each"], exe=exe)[1].count(1) == len(want)
    assert check("splits", *rule_args({"min_run": 1}), act=act, exe=exe) == ["ok %d" % len(sr.scan(act, min_run=1))]


# ------------------------------------------------------------------------------------------------ ABI
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


def test_header_declares_the_symbols():
    txt = open(os.path.join(REPO, "include", "bsrnn_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    want = {
        "bsrnn_hop_activity": ("int", ["bsrnn_ctx*", "constfloat*", "int64_t", "constfloat*", "int64_t", "constint32_t*", "int32_t", "int32_t",
                                       "double*", "void*"]),
        "bsrnn_section_rule_default": ("void", ["bsrnn_section_rule*"]),
        "bsrnn_section_state_reset": ("void", ["bsrnn_section_state*"]),
        "bsrnn_sections_scan": ("int", ["constbsrnn_section_rule*", "bsrnn_section_state*", "constdouble*", "int64_t", "int32_t", "bsrnn_section*",
                                        "int64_t", "int64_t*"]),
    }
    for name, (ret, types) in want.items():
        m = re.search(r"^\s*([A-Za-z_][\w \*]*?)\s+%s\s*\(([^)]*)\)\s*;" % name, body, flags=re.M)
        assert m and m.group(1).strip() == ret, name
        got = [re.sub(r"(?<=[\s\*])[a-zA-Z_]\w*$", "", p.strip()).replace(" ", "") for p in m.group(2).split(",")]
        assert got == types, (name, got)
    assert re.search(r"#define\s+BSRNN_ABI_VERSION\s+2\b", body)
    assert re.search(r"#define\s+BSRNN_ACT_RATIO\s+0\b", body) and re.search(r"#define\s+BSRNN_ACT_LEVEL\s+1\b", body)
    # the contract's words: the reference's script, the deviation, the offset
    assert "gendataset-separate.py" in txt and "math.log(0)" in txt and "est_dev + 1024" in txt


def test_symbols_are_listed_bound_and_exported(native):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (bsrnn_[a-z0-9_]+)", out))
    for name in NEW:
        assert name in native.SYMBOLS and name in exported, name
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert native.lib.bsrnn_hop_activity.argtypes == [vp, vp, i64, vp, i64, ctypes.POINTER(i32), i32, i32, vp, vp]
    assert native.lib.bsrnn_abi_version() == 2
    # the structures are the header's: sizes under the C layout rules
    assert ctypes.sizeof(native.SectionRuleC) == 56 and ctypes.sizeof(native.SectionStateC) == 40 and ctypes.sizeof(native.SectionC) == 24
    rule = native.SectionRuleC()
    native.lib.bsrnn_section_rule_default(ctypes.byref(rule))
    assert [getattr(rule, k) for k, _ in native.SectionRuleC._fields_] == [10.0, 3.0, -30.0, -100.0, 1e-10, -200.0, 10]
    native.lib.bsrnn_section_rule_default(None)
    native.lib.bsrnn_section_state_reset(None)


def test_hop_activity_refusals_without_a_device(native, host_ctx):
    lib = native.lib

    def err():
        return lib.bsrnn_last_error().decode()
    H = 3
    st = H * 1024 + 8
    pool = np.zeros(5 * st, np.float32)                                    # both inputs in one allocation: what lies behind `a` is known
    a, b = pool[:2 * st].reshape(2, st), pool[3 * st:].reshape(2, st)
    act = np.full((2, H, 2), 7.0)
    pa, pb, pact = (x.ctypes.data_as(ctypes.c_void_p) for x in (a, b, act))
    i32s = lambda *v: (ctypes.c_int32 * len(v))(*v)                        # noqa: E731
    call = lib.bsrnn_hop_activity
    assert call(None, pa, st, pb, st, None, 2, H, pact, None) == EARG and "null context" in err()
    for args in ((host_ctx, None, st, pb, st, None, 2, H, pact, None), (host_ctx, pa, st, None, st, None, 2, H, pact, None),
                 (host_ctx, pa, st, pb, st, None, 2, H, None, None)):
        assert call(*args) == EARG and "null argument" in err(), err()
    for R, Hm in ((0, H), (-1, H), (2, 0), (2, -4)):
        assert call(host_ctx, pa, st, pb, st, None, R, Hm, pact, None) == EARG and "R = %d, Hmax = %d" % (R, Hm) in err(), err()
    assert call(host_ctx, pa, H * 1024 - 1, pb, st, None, 2, H, pact, None) == EARG and "mix_stride %d" % (H * 1024 - 1) in err(), err()
    assert call(host_ctx, pa, st, pb, H * 1024 - 1, None, 2, H, pact, None) == EARG and "est_stride %d" % (H * 1024 - 1) in err(), err()
    for bad in (-1, H + 1):
        assert call(host_ctx, pa, st, pb, st, i32s(H, bad), 2, H, pact, None) == EARG
        assert "hops_host[1] = %d" % bad in err() and "[0, %d]" % H in err(), err()
    # the output over an input: the floats the rows span, not one more
    as_d = lambda p, off: ctypes.c_void_p(p.value + off)                  # noqa: E731
    assert call(host_ctx, pa, st, pb, st, None, 2, H, pa, None) == EARG and "overlap" in err(), err()
    assert call(host_ctx, pa, st, pb, st, None, 2, H, pb, None) == EARG and "overlap" in err(), err()
    last = 4 * (st + H * 1024) - 8                                         # the last float of the last row's hops lies in the first double
    assert call(host_ctx, pa, st, pb, st, None, 2, H, as_d(pa, last), None) == EARG and "overlap" in err(), err()
    assert call(host_ctx, pa, st, pb, st, None, 2, H, as_d(pa, last + 8), None) == ESTATE
    # valid arguments: a host-only context cannot compute, and nothing was touched
    assert call(host_ctx, pa, st, pb, st, i32s(0, H), 2, H, pact, None) == ESTATE and "host-only" in err(), err()
    assert call(host_ctx, pa, st, pb, st, None, 2, H, pact, None) == ESTATE
    assert (act == 7.0).all()


def test_sections_scan_refusals_and_sizing(native):
    lib = native.lib

    def err():
        return lib.bsrnn_last_error().decode()
    act = np.array([D] * 11 + [N] + [G] * 12, np.float64)
    pact = act.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    state, out, n = native.SectionStateC(), (native.SectionC * 4)(), ctypes.c_int64(-1)
    lib.bsrnn_section_state_reset(ctypes.byref(state))
    scan_ = lib.bsrnn_sections_scan
    assert scan_(None, None, pact, 24, 1, out, 4, ctypes.byref(n)) == EARG and "null state" in err()
    assert scan_(None, ctypes.byref(state), pact, 24, 1, out, 4, None) == EARG and "null n_out" in err()
    assert scan_(None, ctypes.byref(state), pact, -1, 1, out, 4, ctypes.byref(n)) == EARG and "n_hops = -1" in err()
    assert scan_(None, ctypes.byref(state), pact, 24, 1, out, -2, ctypes.byref(n)) == EARG and "cap = -2" in err()
    assert scan_(None, ctypes.byref(state), None, 24, 1, out, 4, ctypes.byref(n)) == EARG and "act_host is null" in err()
    assert scan_(None, ctypes.byref(state), pact, 24, 1, None, 4, ctypes.byref(n)) == EARG and "out is null" in err()
    rule = native.SectionRuleC()
    lib.bsrnn_section_rule_default(ctypes.byref(rule))
    rule.min_run = 0
    assert scan_(ctypes.byref(rule), ctypes.byref(state), pact, 24, 1, out, 4, ctypes.byref(n)) == EARG and "min_run = 0" in err()
    assert n.value == -1 and state.hop == 0 and state.n_dialog == 0
    # size on a copy of the state with cap = 0, then repeat
    saved = native.SectionStateC.from_buffer_copy(state)
    assert scan_(None, ctypes.byref(saved), pact, 24, 1, None, 0, ctypes.byref(n)) == 0 and n.value == 2
    assert scan_(None, ctypes.byref(state), pact, 24, 1, out, 4, ctypes.byref(n)) == 0 and n.value == 2
    assert [(s.kind, s.first_hop, s.end_hop) for s in out[:2]] == sr.scan(act) == [(1, 9, 11), (2, 21, 24)]
    assert (state.hop, state.open_kind) == (24, 0)
    assert scan_(None, ctypes.byref(state), None, 0, 1, None, 0, ctypes.byref(n)) == 0 and n.value == 0


def test_python_layer_on_the_host(native):
    import inspect
    from speechseparation_amd import mining
    assert list(inspect.signature(mining.hop_activity).parameters) == ["model", "mix", "est", "hops", "out"]
    sig = inspect.signature(mining.mine)
    assert list(sig.parameters) == ["model", "clips", "segment_frames", "max_rows", "rule"]
    assert (sig.parameters["segment_frames"].default, sig.parameters["max_rows"].default) == (256, 64)
    rule = mining.SectionRule()
    assert {k: getattr(rule, k) for k in mining.SectionRule.FIELDS} == sr.DEFAULT_RULE
    with pytest.raises(ValueError):
        mining.SectionRule(min_run=0)
    with pytest.raises(TypeError):
        mining.SectionRule(dialog=3)
    # the scanner is the C state: split feeds, flush, reset, a non-default rule
    act = sequence(11)
    want = sr.scan(act)
    sc = mining.SectionScanner()
    got = sc.feed(act[:100]) + sc.feed(act[100:101]) + sc.feed(act[101:]) + sc.flush()
    assert [tuple(s) for s in got] == want and sc.hop == len(act) and sc.open is None and sc.flush() == []
    assert all(s.samples == (s.first_hop * 1024, s.end_hop * 1024) and s.name in ("dialog", "background") for s in got)
    sc.reset()
    assert sc.hop == 0 and [tuple(s) for s in sc.feed(act, flush=True)] == want
    sc = mining.SectionScanner(mining.SectionRule(min_run=1, silence_db=-210.0))
    assert [tuple(s) for s in sc.feed(act) + sc.flush()] == sr.scan(act, min_run=1, silence_db=-210.0)
    sc = mining.SectionScanner()
    assert sc.feed(np.array([D] * 12)) == [] and sc.open == (1, 9)
    with pytest.raises(ValueError):
        sc.feed(np.zeros((3, 3)))
