"""Shapes, data and gates shared by tests/test_lcsd_host.py (the host build of csrc/lpsd.h's pair
forms) and tests/test_gpu_lcsd.py (the kernels): both are held to the same numbers.

Shapes, means and orders: those of lpsd_cases.py (s1, s2, s3; mean 0 / -1 / 100; order 0 / -1).
Data: x = lpsd_cases.series(shape, mean, seed=1),
      y = 0.5 mean + 0.7 (x - mean) + 1e-3 RandomState(2).randn(N)
(a part coherent with x plus independent noise of x's own size: the coherence runs from
0.005 at the many-segment frequencies to 1 at K = 1).

Gates (per case, DESIGN.md §13's rule): the deviation of the float64 restatement (lcsd_ref.lcsd)
from its longdouble twin, times GATE_MARGIN = 16, and never less than 1e-12; the code under test
is held to that, measured against the longdouble twin. The deviation measures:
  Sxx, Syy  max_j |S / S_ref - 1|                     (relative, as §13)
  Sxy       max_j |Sxy - Sxy_ref| / sqrt(Sxx Syy)     (Sxy may be near 0: a relative gate would
                                                        be meaningless)
  coh       max_j |coh - coh_ref|                     (absolute)
float64-to-longdouble deviations: Sxy 1.4e-15 .. 1.8e-14 at mean 0, 2.6e-13 .. 2.8e-12 at
mean -1, 7e-11 .. 2.4e-10 at mean 100; coh <= 1.7e-15, 5.8e-13, 5.8e-11."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lcsd_ref as R  # noqa: E402
import lpsd_cases as LC  # noqa: E402

FS, SHAPES, MEANS, ORDERS, CASES, KNOWN = LC.FS, LC.SHAPES, LC.MEANS, LC.ORDERS, LC.CASES, LC.KNOWN
GATE_MARGIN, GATE_FLOOR = 16.0, 1e-12
settings = LC.settings
QUANTITIES = ("Sxx", "Syy", "Sxy", "coh")


def pair(shape, mean):
    x = LC.series(shape, mean, seed=1)
    y = 0.5 * mean + 0.7 * (x - mean) + 1e-3 * np.random.RandomState(2).randn(SHAPES[shape]["N"])
    return x, y


def deviations(got, ref):
    """The four deviation measures of `got` (a dict or an object with Sxx, Syy, Sxy, coh) from
    the longdouble result `ref`."""
    g = got if isinstance(got, dict) else got._asdict()
    ld = np.longdouble
    scale = np.sqrt(ref["Sxx"] * ref["Syy"])
    return dict(
        Sxx=float(np.max(np.abs(np.asarray(g["Sxx"]).astype(ld) / ref["Sxx"] - 1))),
        Syy=float(np.max(np.abs(np.asarray(g["Syy"]).astype(ld) / ref["Syy"] - 1))),
        Sxy=float(np.max(np.abs(np.asarray(g["Sxy"]).astype(np.clongdouble) - ref["Sxy"]) / scale)),
        coh=float(np.max(np.abs(np.asarray(g["coh"]).astype(ld) - ref["coh"]))))


@functools.lru_cache(maxsize=None)
def reference(shape, mean, order):
    """(x, y, longdouble-twin result, gates) of a case; computed once, read-only."""
    x, y = pair(shape, mean)
    r64 = R.lcsd(x, y, FS, order=order, **settings(shape))
    rld = R.lcsd(x, y, FS, order=order, dtype=np.longdouble, **settings(shape))
    dev = deviations(r64, rld)
    gates = {q: max(GATE_MARGIN * dev[q], GATE_FLOOR) for q in QUANTITIES}
    for a in (x, y) + tuple(v for v in rld.values()):
        a.setflags(write=False)
    return x, y, rld, gates


def ratios(got, shape, mean, order):
    """Each deviation of `got` from the longdouble twin over the case's gate."""
    _, _, ref, gates = reference(shape, mean, order)
    dev = deviations(got, ref)
    return {q: dev[q] / gates[q] for q in QUANTITIES}


# known answer: two sines at a plan frequency of lpsd_cases.KNOWN, y 0.4 x as large and 1.1 rad behind
KNOWN_Y = dict(amp=0.004, offset=-1.0, lag=1.1)


def known_pair(j):
    p = R.plan(KNOWN["N"], FS, Jdes=KNOWN["Jdes"])
    assert p[2][j] >= 9.0
    t = np.arange(KNOWN["N"]) / FS
    ph = 2 * np.pi * p[0][j] * t + KNOWN["phase"]
    return KNOWN["offset"] + KNOWN["amp"] * np.sin(ph), KNOWN_Y["offset"] + KNOWN_Y["amp"] * np.sin(ph - KNOWN_Y["lag"])


def check_known(Sxy, H, coh, enbw, j):
    """The three known-answer figures at frequency j: (Sxy ENBW / (Ax Ay / 2 e^{-i lag}) - 1,
    |H - 0.4 e^{-i lag}|, |coh - 1|), each to be within KNOWN['tol']."""
    e = np.exp(-1j * KNOWN_Y["lag"])
    return (abs(Sxy[j] * enbw[j] / (KNOWN["amp"] * KNOWN_Y["amp"] / 2 * e) - 1),
            abs(H[j] - KNOWN_Y["amp"] / KNOWN["amp"] * e), abs(coh[j] - 1))


# statistics: white x and independent n of the same variance, N = 20000, Jdes 100
STAT = dict(N=20000, Jdes=100, sigma=1e-3, Kmin=50)


def stat_series():
    return (STAT["sigma"] * np.random.RandomState(0).randn(STAT["N"]),
            STAT["sigma"] * np.random.RandomState(1).randn(STAT["N"]))


def check_statistics(indep, summed, K):
    """indep = lcsd(x, n), summed = lcsd(x, x + n) as (coh, H, resid) each; asserts the issue's
    bounds over the frequencies with K >= 50 and at the K = 1 frequency; returns the figures."""
    many = K >= STAT["Kmin"]
    assert many.sum() == 51 and (K == 1).sum() == 1
    fig = dict(indep_coh=float(np.median(indep[0][many])), coh=float(np.median(summed[0][many])),
               absH=float(np.median(np.abs(summed[1][many]))),
               resid=float(np.median(summed[2][many] / (2 * STAT["sigma"] ** 2 / FS))))
    print("statistics:", ", ".join(f"{k} {v:.4f}" for k, v in fig.items()))
    assert fig["indep_coh"] <= 0.05
    assert 0.4 <= fig["coh"] <= 0.6
    assert 0.9 <= fig["absH"] <= 1.1
    assert 0.9 <= fig["resid"] <= 1.1
    assert abs(indep[0][K == 1][0] - 1) <= 1e-12 and abs(summed[0][K == 1][0] - 1) <= 1e-12
    return fig
