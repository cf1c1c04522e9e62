"""Shapes, data and gates shared by tests/test_lpsd_host.py (the host build of csrc/lpsd.h) and
tests/test_gpu_lpsd.py (the kernels): both are held to the same numbers.

Shapes: the smallest that reach every branch of the kernels.
  s1  N = 500, Jdes 100, fs 50: J = 27, L 28..500, K 1..73 — K = 1 => L = N, segments shorter
      than a wave, lengths that are no multiple of 64, both sides of the 256-sample threshold
      between one wave and one workgroup per segment
  s2  the same with Lmin = 64 and bmin = 2.5 (three of its frequencies take the bin floor)
  s3  N = 4096, Jdes 60: segments of several strides of a 256-lane workgroup, K up to 1090
Data: mean + 1e-3 randn, mean in {0, -1, 100}, order 0 and -1.

Gate (per case): the relative deviation of Sxx between the float64 restatement
(lpsd_ref.lpsd) and its longdouble twin on the same data measures what float64 arithmetic
costs on that data (1e-15 at mean 0, ~1e-10 at mean 100, where the window's 200 dB of
side-lobe suppression meet a mean 1e5 times the noise). The code under test sums in another
order and has its own I0 and sincos, so it gets 16 x that deviation, and never less than
1e-12. The figure compared with the gate is the largest relative deviation from the
longdouble twin over the plan's frequencies."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpsd_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FS = 50.0
SHAPES = {
    "s1": dict(N=500, Jdes=100),
    "s2": dict(N=500, Jdes=100, Lmin=64, bmin=2.5),
    "s3": dict(N=4096, Jdes=60),
}
MEANS = (0.0, -1.0, 100.0)
ORDERS = (0, -1)
CASES = [(s, m, o) for s in SHAPES for m in MEANS for o in ORDERS]
GATE_MARGIN, GATE_FLOOR = 16.0, 1e-12


def settings(shape):
    kw = dict(SHAPES[shape])
    kw.pop("N")
    return kw


def series(shape, mean, seed=1):
    return mean + 1e-3 * np.random.RandomState(seed).randn(SHAPES[shape]["N"])


@functools.lru_cache(maxsize=None)
def reference(shape, mean, order):
    """(x, longdouble-twin Sxx as float64, enbw, gate) of a case; computed once, read-only."""
    x = series(shape, mean)
    r64 = R.lpsd(x, FS, order=order, **settings(shape))
    rld = R.lpsd(x, FS, order=order, dtype=np.longdouble, **settings(shape))
    dev = float(np.max(np.abs(r64["Sxx"].astype(np.longdouble) / rld["Sxx"] - 1)))
    gate = max(GATE_MARGIN * dev, GATE_FLOOR)
    sxx = rld["Sxx"].astype(np.float64)
    enbw = rld["enbw"].astype(np.float64)
    for a in (x, sxx, enbw):
        a.setflags(write=False)
    return x, sxx, enbw, gate


def ratio(sxx, shape, mean, order):
    """Largest relative deviation of sxx from the longdouble twin, over the case's gate."""
    _, ref, _, gate = reference(shape, mean, order)
    return float(np.max(np.abs(sxx / ref - 1))) / gate


# known answer: a sine at a plan frequency; Sxx ENBW = A^2/2 where the bin is clear of the
# image's main lobe (b >= 9)
KNOWN = dict(N=20000, Jdes=100, amp=0.01, offset=2.5, phase=0.3, js=(25, 40, 50), tol=1e-9)


def known_series(j):
    p = R.plan(KNOWN["N"], FS, Jdes=KNOWN["Jdes"])
    assert p[2][j] >= 9.0
    t = np.arange(KNOWN["N"]) / FS
    return KNOWN["offset"] + KNOWN["amp"] * np.sin(2 * np.pi * p[0][j] * t + KNOWN["phase"])
