"""A restatement, in numpy, of the two rules of the section mining (include/bsrnn_hip.h, bsrnn_hop_activity and bsrnn_sections_scan),
written from their description: the per-hop figures with float32 terms and float64 sums, and the run-length state machine over them.
The tests compare the kernel, the host header and the Python layer against it."""
import math

import numpy as np

HOP = 1024
DIALOG, BACKGROUND = 1, 2
DEFAULT_RULE = dict(dialog_db=10.0, bridge_db=3.0, background_db=-30.0, silence_db=-100.0, level_floor=1e-10, floor_db=-200.0, min_run=10)
REL = 1e-12          # two float64 sums of the same 1024 non-negative terms in different orders: each within 1023 * 2^-53 = 1.1e-13


def activity(mix, est, hops=None, n_hops=None):
    """mix, est: float32 [R, >= H * 1024] -> float64 [R, H, 2]; rows with hops[r] < H hold (0, 0) from hops[r] on and are not read there."""
    mix, est = np.asarray(mix, np.float32), np.asarray(est, np.float32)
    R = mix.shape[0]
    H = n_hops if n_hops is not None else min(mix.shape[1], est.shape[1]) // HOP
    out = np.zeros((R, H, 2), np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        for r in range(R):
            hr = H if hops is None else int(hops[r])
            w = mix[r, :hr * HOP].reshape(hr, HOP)
            e = est[r, :hr * HOP].reshape(hr, HOP)
            b = w - e                                                     # float32
            q = (e * e) / (b * b)                                         # float32: two products, one IEEE division
            s = w * w
            assert b.dtype == q.dtype == s.dtype == np.float32
            out[r, :hr, 0] = q.astype(np.float64).sum(axis=1) / HOP
            out[r, :hr, 1] = s.astype(np.float64).sum(axis=1) / HOP
    return out


def to_db(ratio):
    if ratio == 0.0:
        return -math.inf
    if math.isnan(ratio) or math.isinf(ratio):
        return ratio
    return 10.0 * math.log(ratio)


def to_level(level_mean, rule):
    if level_mean < rule["level_floor"]:
        return rule["floor_db"]
    if math.isnan(level_mean) or math.isinf(level_mean):
        return level_mean
    return 10.0 * math.log(level_mean)


class Scanner:
    def __init__(self, **rule):
        self.rule = dict(DEFAULT_RULE, **rule)
        self.reset()

    def reset(self):
        self.n_dialog = self.n_background = 0
        self.open = None                     # (kind, first_hop)
        self.hop = 0

    def _close(self, out):
        if self.open is not None:
            out.append((self.open[0], self.open[1], self.hop))
            self.open = None

    def feed(self, act, flush=False):
        q, out = self.rule, []
        for ratio, level_mean in np.asarray(act, np.float64).reshape(-1, 2):
            db, level = to_db(float(ratio)), to_level(float(level_mean), q)
            if db > q["dialog_db"]:
                if self.n_background > 0:
                    self.n_background = 0
                    self._close(out)
                self.n_dialog += 1
                if self.n_dialog >= q["min_run"] and self.open is None:
                    self.open = (DIALOG, self.hop)
            elif (db > q["bridge_db"] or level < q["silence_db"]) and self.n_dialog >= q["min_run"]:
                pass
            elif db < q["background_db"]:
                if self.n_dialog > 0:
                    self.n_dialog = 0
                    self._close(out)
                self.n_background += 1
                if self.n_background >= q["min_run"] and self.open is None:
                    self.open = (BACKGROUND, self.hop)
            else:
                self.n_dialog = self.n_background = 0
                self._close(out)
            self.hop += 1
        if flush:
            self._close(out)
        return out


def scan(act, **rule):
    """The sections of one row's activity [n, 2], flushed at its end."""
    return Scanner(**rule).feed(act, flush=True)


def finite_dbs(act):
    a = np.asarray(act, np.float64).reshape(-1, 2)[:, 0]
    return np.array([to_db(float(v)) for v in a if np.isfinite(v) and v != 0.0])


def clear_of_thresholds(act, margin=1e-6, **rule):
    """No finite db of the activity lies within `margin` of one of the three db thresholds."""
    q = dict(DEFAULT_RULE, **rule)
    d = finite_dbs(act)
    return all((np.abs(d - q[k]) > margin).all() for k in ("dialog_db", "bridge_db", "background_db"))


def compare_activity(got, want, what=""):
    """Finite values at REL; inf, NaN and exact 0 exactly, by position.  Prints the largest relative difference before it asserts."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    special = ~np.isfinite(want) | (want == 0.0)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not np.isneginf(got).any(), what
    assert np.array_equal(got == 0.0, want == 0.0), what
    ok = ~special
    rel = float((np.abs(got[ok] - want[ok]) / np.abs(want[ok])).max()) if ok.any() else 0.0
    print("%s: %d finite values, max relative difference %.3e (bound %.1e)" % (what, int(ok.sum()), rel, REL))
    assert rel <= REL, (what, rel)
    return rel
