"""Every dual-path kernel variant at the fp32 rounding bound, with carried state in and out.

BSRNN.dual_path(z, state) (bsrnn_dual_path: the four recurrent blocks of the model's own schedule) runs in a child process per
knob set (the knobs of plan_call, csrc/plan_host.h, are read once per process by csrc/api.hip) at the smallest shapes that cross each decision and tile
edge of the band-axis and time-axis kernels of csrc/lstm.hip.  Both outputs, z_out and state_out, are held on all rows to the
criterion of test_gpu_parity.py::test_precision_is_at_fp32_rounding_level,
    e_hip <= 3 * e_f32 + 1e-7,
e_hip: the largest distance of the HIP result from the float64 numpy oracle, e_f32: the float32 numpy oracle's distance from it on
the same case.  A witness per child (launch counts of the band_fc / time_fc stages of one profiled call) proves that the knob set
changed the flow, and the two bit relations that the knobs promise (eight sequences per workgroup == four; grouped-GEMM fc after the
pair launch == one launch per layer) are checked on the same arrays.  A CPU test holds an independent float32 evaluation (the torch
CPU oracle) to the same criterion on the same cases: the bound is fair where float32 arithmetic itself meets it."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import REPO

CHILD_TIMEOUT = 300      # seconds per child; a child takes 10 - 20 s (process start and weight packing)


def case(name, C, T, tab="12", w="default", kind="dual"):
    return dict(name=name, C=C, T=T, table=tab, w=w, kind=kind)


# The default 12-band table unless named; weights alternate between the suite's sd_default and sd_hot (lstm_gain = 3, saturating gates).
# At most five models per child: 12 / default, 12 / hot, 41 / hot, K=16 / default, K=17 / hot.
CASES = [
    # the small band block (M = C T <= 8, four band sequences per workgroup): one sequence, a partial second workgroup, two full ones
    case("1x1", 1, 1), case("5x1", 5, 1, w="hot"), case("2x4", 2, 4),
    # first call past it: the pair launch with one partial tile of 16
    case("3x3", 3, 3, w="hot"),
    # band tiles and groups: M = 16, 17, 128 (eight tiles: one full group of 16 workgroups), 129
    case("1x16", 1, 16), case("1x17", 1, 17, w="hot"), case("2x64", 2, 64), case("3x43", 3, 43, w="hot"),
    # time axis: 4-step input groups with layer 1 running behind; the 8-step staging of the 8-sequence kernel (TCH8, RING8)
    case("1x2", 1, 2), case("1x3", 1, 3, w="hot"), case("1x4", 1, 4), case("1x5", 1, 5, w="hot"), case("1x7", 1, 7),
    case("1x8", 1, 8, w="hot"), case("1x9", 1, 9),
    # time axis: the 16-step h0 / h1 rings (H0RING, H1RING)
    case("1x15", 1, 15, w="hot"), case("1x31", 1, 31), case("1x32", 1, 32, w="hot"), case("1x33", 1, 33),
    # many ring wraps and drift
    case("1x1024", 1, 1024, w="hot"),
    # a mid-size batch
    case("11x40", 11, 40),
    # the automatic switch to eight sequences per workgroup, (C K + 3) / 4 > CUs: 255 and 258 workgroups of four against the 256 CUs of
    # an MI355X (on a part with another CU count both cases still run and are checked, on whichever kernel plan_call picks)
    case("85x3", 85, 3, w="hot"), case("86x3", 86, 3),
    # 41-band table (K = 42): a partial last time-axis workgroup, N % 4 = 2 and N % 8 = 2 (N = 42), 6 (N = 126), 2 (N = 42)
    case("41 1x9", 1, 9, tab="41", w="hot"), case("41 3x5", 3, 5, tab="41", w="hot"), case("41 1x40", 1, 40, tab="41", w="hot"),
    # the K <= 16 condition of the small band block
    case("K16 2x3", 2, 3, tab="K=16"), case("K17 2x3", 2, 3, tab="K=17", w="hot"), case("K16 2x4", 2, 4, tab="K=16"),
    # no state in (zero initial state), state out checked
    case("nostate 2x6", 2, 6, kind="nostate"),
    # chained: the state out of a T = 5 call feeds a T = 11 call
    case("chain 2x5+11", 2, 5, w="hot", kind="chain"),
]
CHAIN_T2 = 11

# Knob sets -> environment and the witness (which of the band_fc / time_fc stages must have launches).  Every child also runs under
# BSRNN_OVERLAP=0 (bsrnn_dual_path never overlaps; this keeps the children alike).
KNOB_NAMES = ("BSRNN_TIME_SEQ8", "BSRNN_BAND_FC", "BSRNN_BAND_PAIR", "BSRNN_TIME_KERNEL", "BSRNN_GEMM", "BSRNN_LSTM", "BSRNN_MLP")
KNOBS = {
    "default": dict(env={}, band_fc=False, time_fc=False),
    "seq8": dict(env={"BSRNN_TIME_SEQ8": "1"}, band_fc=False, time_fc=False),
    "fc_gemm": dict(env={"BSRNN_BAND_FC": "gemm"}, band_fc=True, time_fc=None),
    "layers": dict(env={"BSRNN_BAND_PAIR": "0"}, band_fc=True, time_fc=None),
    "v3": dict(env={"BSRNN_TIME_KERNEL": "v3"}, band_fc=None, time_fc=True),
    "gemm_f32": dict(env={"BSRNN_GEMM": "f32"}, band_fc=None, time_fc=True),
}


def table(name):
    from speechseparation_amd import spec
    if name in ("12", "41"):
        return spec.variant_bandsplits("41" if name == "41" else "default")
    from test_gpu_band_tables import BAND_COUNT_TABLES
    return BAND_COUNT_TABLES[name]


_SD = {}


def state_dict(name, w):
    """Weights per (table, set): on the 12-band table the suite's sd_default / sd_hot."""
    from speechseparation_amd import weights
    key = (name, w)
    if key not in _SD:
        v = None if name == "12" else table(name)
        seed = (0 if w == "default" else 1) + {"12": 0, "41": 3, "K=16": 6, "K=17": 9}[name]
        _SD[key] = weights.synth_state_dict(v, seed=seed, lstm_gain=3.0 if w == "hot" else 1.0)
    return _SD[key]


def inputs(c):
    """The numpy inputs of a case, from seeds."""
    from speechseparation_amd import weights
    seed = 30000 + 100 * CASES.index(c)
    K = len(table(c["table"]))
    d = {"z": weights.synth_tensor((c["C"], c["T"], K, 64), seed=seed, scale=1.0)}
    if c["kind"] != "nostate":
        d["s"] = weights.synth_tensor((4, 2, c["C"] * K, 64), seed=seed + 9, scale=0.5)
    if c["kind"] == "chain":
        d["z2"] = weights.synth_tensor((c["C"], CHAIN_T2, K, 64), seed=seed + 1, scale=1.0)
    return d


def run_steps(c, arr, step):
    """The case's call(s) through `step(z, state or None) -> (z_out, state_out)` -> dict of outputs."""
    if c["kind"] == "chain":
        z1, s1 = step(arr["z"], arr["s"])
        z2, s2 = step(arr["z2"], s1)
        return {"z": z1, "z2": z2, "state": s2}
    z, s = step(arr["z"], arr.get("s"))
    return {"z": z, "state": s}


def run_case(m, c, arr):
    """On the model `m` (cuda) -> dict of numpy outputs."""
    cu = {k: torch.from_numpy(a).cuda() for k, a in arr.items()}
    out = run_steps(c, cu, lambda z, s: m.dual_path(z, s))
    return {k: a.cpu().numpy() for k, a in out.items()}


def make_model(tab, w):
    from speechseparation_amd.bsrnn import BSRNN
    m = BSRNN(None if tab == "12" else table(tab)).eval()
    m.load_state_dict({k: torch.from_numpy(a.copy()) for k, a in state_dict(tab, w).items()}, strict=True)
    return m.to("cuda")


def oracle(c, arr, dtype):
    """The numpy oracle of a case in `dtype`, keyed like run_case's outputs."""
    from oracle import bsrnn_numpy as onp
    sd = state_dict(c["table"], c["w"])
    return run_steps(c, arr, lambda z, s: onp.dual_path(sd, z.astype(dtype), None if s is None else s.astype(dtype), dtype))


_TORCH = {}


def torch_oracle(c, arr):
    """The torch CPU oracle (stock nn.LSTM / addmm) of a case in float32."""
    from oracle.bsrnn_torch_cpu import TorchCpuBSRNN
    key = (c["table"], c["w"])
    if key not in _TORCH:
        _TORCH[key] = TorchCpuBSRNN(state_dict(*key), table(c["table"]))
    ref = _TORCH[key]

    def step(z, s):
        with torch.no_grad():
            return ref._dual_path(torch.as_tensor(z), None if s is None else torch.as_tensor(s))
    return {k: a.contiguous().numpy() for k, a in run_steps(c, arr, step).items()}


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def shape_text(c):
    return "C=%d T=%d%s" % (c["C"], c["T"], "+%d" % CHAIN_T2 if c["kind"] == "chain" else "")


def references(cases=None, say=None):
    """{case name: (float64 outputs, float32 outputs)} of the numpy oracle."""
    out = {}
    for c in cases or CASES:
        arr = inputs(c)
        out[c["name"]] = (oracle(c, arr, np.float64), oracle(c, arr, np.float32))
        if say:
            say(c["name"])
    return out


def report(label, got, refs, cases=None):
    """One line per case and output of `got(case) -> {output: array}` against `refs`; -> (lines, failures, worst ratio per output
    class 'z' / 'state').  The criterion is the suite's rounding-level bound and is not tuned to what the kernels give."""
    lines, bad, worst = [], [], {"z": 0.0, "state": 0.0}
    for c in cases or CASES:
        r64, r32 = refs[c["name"]]
        res = got(c)
        for key in r64:
            hip = res[key]
            assert hip.shape == r64[key].shape, (c["name"], key, hip.shape, r64[key].shape)
            e_hip, e_f32 = maxabs(hip, r64[key]), maxabs(r32[key], r64[key])
            bound = 3 * e_f32 + 1e-7
            ok = bool(np.isfinite(hip).all()) and e_hip <= bound
            cls = "state" if key == "state" else "z"
            worst[cls] = max(worst[cls], e_hip / bound)
            lines.append("dual path %-9s %-13s K=%-2d %-13s %-7s %-6s e_hip %.2e  e_f32 %.2e  bound %.2e%s" % (
                label, c["name"], len(table(c["table"])), shape_text(c), c["w"], key, e_hip, e_f32, bound, "" if ok else "  FAIL"))
            if not ok:
                bad.append((c["name"], key, e_hip, e_f32))
    lines.append("dual path %-9s worst e / bound: z %.2f  state %.2f" % (label, worst["z"], worst["state"]))
    return lines, bad, worst


@pytest.fixture(scope="module")
def refs():
    """The float64 and float32 numpy oracles of every case, computed once for all tests of the module (read-only)."""
    return references()


# -------------------------------------------------------------------------------------------------------------------- CPU: the bound is fair
def test_bound_is_fair_for_an_independent_float32_evaluation(refs):
    """The torch CPU oracle in float32, a second float32 evaluation with its own operation order (MKLDNN RNN, addmm), meets the
    criterion on every case and output: the case list holds no case where float32 arithmetic itself is unstable."""
    lines, bad, _ = report("torch-cpu", lambda c: torch_oracle(c, inputs(c)), refs)
    print("\n".join(lines))
    assert not bad, bad


# -------------------------------------------------------------------------------------------------------------------- GPU children
CHILD = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[2])
from speechseparation_amd import _native
from test_gpu_dual_path_precision import CASES, inputs, run_case, make_model
mode = _native.compute_mode()
assert mode["lstm"] == "fp16x2" and mode["gemm"] == sys.argv[3], mode
out, models = {}, {}
for c in CASES:
    key = (c["table"], c["w"])
    if key not in models:
        models[key] = make_model(*key)
    for k, a in run_case(models[key], c, inputs(c)).items():
        out[c["name"] + "/" + k] = a
    print("ran", c["name"], flush=True)
# witness: the stages of one profiled (3, 3) call
c = [c for c in CASES if c["name"] == "3x3"][0]
m = models[(c["table"], c["w"])]
m.set_profiling(True)
m.stage_times(reset=True)
run_case(m, c, inputs(c))
out["witness"] = np.frombuffer(json.dumps({k: v[1] for k, v in m.stage_times(reset=True).items()}).encode(), dtype=np.uint8)
m.set_profiling(False)
np.savez(sys.argv[1], **out)
print("done", flush=True)
'''


class Children:
    """Runs the child of a knob set on first use, one at a time.  Once a child has ended other than by exit status 0 (a signal, an
    abort, its timeout, an error), no further child is started: every test that still needs one fails with that child's output."""

    def __init__(self, directory):
        self.dir = directory
        self.done = {}
        self.dead = None

    def get(self, knob):
        if knob in self.done:
            return self.done[knob]
        assert self.dead is None, "no child started after this one:\n" + self.dead
        path = os.path.join(self.dir, knob + ".npz")
        env = {k: v for k, v in os.environ.items() if k not in KNOB_NAMES}
        env.update(KNOBS[knob]["env"], PYTHONPATH=REPO, BSRNN_OVERLAP="0")
        cmd = [sys.executable, "-c", CHILD, path, os.path.join(REPO, "tests"), env.get("BSRNN_GEMM", "fp16x2")]
        try:
            r = subprocess.run(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
            rc, text = r.returncode, r.stdout
        except subprocess.TimeoutExpired as e:
            text = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
            rc = "timeout after %d s" % CHILD_TIMEOUT
        if rc != 0:
            self.dead = "child '%s' ended with %s\n%s" % (knob, rc, text[-3000:])
            raise AssertionError(self.dead)
        self.done[knob] = dict(np.load(path))
        return self.done[knob]


@pytest.fixture(scope="module")
def children():
    with tempfile.TemporaryDirectory() as d:
        yield Children(d)


def check_knob_set(knob, children, refs):
    res = children.get(knob)
    lines, bad, _ = report(knob, lambda c: {k: res[c["name"] + "/" + k] for k in refs[c["name"]][0]}, refs)
    print("\n".join(lines))
    counts = json.loads(bytes(res["witness"]).decode())
    print("dual path %-9s witness (3, 3): launches %s" % (knob, {k: counts[k] for k in ("band_lstm", "band_fc", "time_lstm", "time_fc")}))
    assert counts["band_lstm"] > 0 and counts["time_lstm"] > 0, counts
    for stage in ("band_fc", "time_fc"):
        want = KNOBS[knob][stage]
        if want is not None:
            assert (counts[stage] > 0) == want, (knob, stage, counts)
    assert not bad, bad


def check_same_bits(a, b, children):
    ra, rb = children.get(a), children.get(b)
    diff = [(k, maxabs(ra[k], rb[k])) for k in ra if k != "witness" and not np.array_equal(ra[k], rb[k])]
    assert set(ra) == set(rb) and len(ra) > 2 * len(CASES)
    assert not diff, diff


@pytest.mark.gpu
def test_shipped_flow(children, refs):
    """No knob: band_block_small_kernel, band_pair_h2_kernel<true>, time_lstm_h2w_kernel<true, ., PART>; time_lstm_h2w8_kernel at C = 86."""
    check_knob_set("default", children, refs)


@pytest.mark.gpu
def test_eight_sequences_per_workgroup(children, refs):
    """BSRNN_TIME_SEQ8=1: time_lstm_h2w8_kernel at every shape, partial workgroups of 2, 4 and 6 sequences; without PART at M <= 8."""
    check_knob_set("seq8", children, refs)


@pytest.mark.gpu
def test_pair_launch_with_gemm_fc(children, refs):
    """BSRNN_BAND_FC=gemm: band_pair_h2_kernel<false>, the band block's fc as a grouped gemm_h2 launch, the fused time kernel without PART."""
    check_knob_set("fc_gemm", children, refs)


@pytest.mark.gpu
def test_one_launch_per_band_layer(children, refs):
    """BSRNN_BAND_PAIR=0: band_lstm_h2_kernel<64> and <128>."""
    check_knob_set("layers", children, refs)


@pytest.mark.gpu
def test_unfused_time_kernel(children, refs):
    """BSRNN_TIME_KERNEL=v3: time_lstm_h2w_kernel<false> and the time block's fc as a launch of its own."""
    check_knob_set("v3", children, refs)


@pytest.mark.gpu
def test_fp16x2_recurrence_around_exact_fc(children, refs):
    """BSRNN_GEMM=f32 with the default BSRNN_LSTM: the fp16x2 recurrent kernels around exact-fp32 fc launches; no small band block, no fc
    inside the time kernel."""
    check_knob_set("gemm_f32", children, refs)


@pytest.mark.gpu
def test_eight_sequences_equal_four_bit_for_bit(children):
    """Every case, the N % 8 tails and the T edges included: BSRNN_TIME_SEQ8=1 gives the bits of the shipped flow."""
    check_same_bits("seq8", "default", children)


@pytest.mark.gpu
def test_gemm_fc_after_the_pair_launch_equals_one_launch_per_layer_bit_for_bit(children):
    """Every case: BSRNN_BAND_FC=gemm gives the bits of BSRNN_BAND_PAIR=0 (the same arithmetic on the same numbers)."""
    check_same_bits("fc_gemm", "layers", children)
