#!/usr/bin/env python3
"""Measurement: distance of the dual-path step (4 recurrent blocks) of a library build to the float64 oracle,
beside the float32 oracle's own distance (same inputs as tests/test_gpu_parity.py::test_precision_is_at_fp32_rounding_level),
then the table of tests/test_gpu_dual_path_precision.py (its case list, z_out and state_out, e_hip against 3 e_f32 + 1e-7) for
that library under the knobs of this process's environment.
    BSRNN_HIP_LIB=build/ab/variant.so python tools/precision_dual_path.py
    BSRNN_HIP_LIB=build/ab/variant.so BSRNN_TIME_SEQ8=1 python tools/precision_dual_path.py
Exit status 1 if a case misses the bound.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import bsrnn_numpy as orc          # noqa: E402  (checker)
from speechseparation_amd import weights      # noqa: E402
from speechseparation_amd.bsrnn import BSRNN   # noqa: E402
import test_gpu_dual_path_precision as grid    # noqa: E402  (the case list and the table)

for label, kw in (("default", dict(seed=0)), ("hot", dict(seed=1, lstm_gain=3.0))):
    sd = weights.synth_state_dict(None, **kw)
    m = BSRNN().eval()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m = m.to("cuda:0")
    for seed in (78, 79, 80):
        z = weights.synth_tensor((3, 24, 12, 64), seed=seed, scale=1.0)
        z64, _ = orc.dual_path(sd, z.astype(np.float64), None, np.float64)
        z32, _ = orc.dual_path(sd, z, None, np.float32)
        zo, _ = m.dual_path(torch.from_numpy(z).cuda())
        zo = zo.cpu().numpy()
        print("%s %-8s seed %d  |hip - f64| %.2e   |f32 oracle - f64| %.2e   max|z| %.2f"
              % (os.environ.get("BSRNN_HIP_LIB", "in-tree"), label, seed, np.abs(zo - z64).max(), np.abs(z32 - z64).max(), np.abs(z64).max()))
    del m

knobs = " ".join("%s=%s" % (k, os.environ[k]) for k in grid.KNOB_NAMES + ("BSRNN_OVERLAP",) if k in os.environ) or "no knob"
print("%s, %s" % (os.environ.get("BSRNN_HIP_LIB", "in-tree"), knobs))
models = {}


def run(c):
    key = (c["table"], c["w"])
    if key not in models:
        models[key] = grid.make_model(*key)
    return grid.run_case(models[key], c, grid.inputs(c))


lines, bad, _ = grid.report("tool", run, grid.references())
print("\n".join(lines))
sys.exit(1 if bad else 0)
