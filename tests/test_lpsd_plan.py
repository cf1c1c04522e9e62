"""dfmi_lpsd_plan (csrc/lpsd_plan.h, host only) against the numpy restatement
tests/helpers/lpsd_ref.plan over a grid of settings: J, L and K exactly, f, fres and b within
4 ulp (both are double arithmetic in the same order; the margin covers a libm pow / sqrt that
differs in the last place); the plan's invariants; every rejected argument. CPU only."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lpsd_ref as R  # noqa: E402

FS = 50.0
GRID = list(itertools.product((8, 500, 4096, 20000, 10**7), (27, 100, 500), (1, 100), (1, 2.5), (0, 64),
                              ("default", 0, 0.5)))


def _plan(N, fs=FS, olap="default", bmin=1, Lmin=0, Jdes=500, Kdes=100):
    from deepfmkit_amd import lpsd as M
    return M.plan(N, fs, olap=olap, bmin=bmin, Lmin=Lmin, Jdes=Jdes, Kdes=Kdes)


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("N", [8, 500, 4096, 20000, 10**7])
def test_plan_matches_the_restatement_and_keeps_its_invariants(N):
    worst = 0.0
    for n, Jdes, Kdes, bmin, Lmin, olap in GRID:
        if n != N:
            continue
        kw = dict(olap=olap, bmin=bmin, Lmin=Lmin, Jdes=Jdes, Kdes=Kdes)
        p = _plan(N, **kw)
        f, fres, b, L, K = R.plan(N, FS, **kw)
        assert p.f.size == f.size, kw
        assert np.array_equal(p.L, L) and np.array_equal(p.K, K), kw
        for ours, ref in ((p.f, f), (p.fres, fres), (p.b, b)):
            if ref.size:
                worst = max(worst, float(_ulps(ours, ref).max()))
        if p.f.size == 0:
            continue
        assert (np.diff(p.f) > 0).all() and p.f[-1] < FS / 2, kw
        assert (p.L >= 1).all() and (p.L <= N).all() and (p.K >= 1).all(), kw
        assert (p.L[p.K == 1] == N).all(), kw
        assert (p.b >= bmin).all(), kw
        # the last segment ends inside the series (segment k starts at floor(k (N-L)/(K-1) + 0.5))
        many = p.K > 1
        last = np.floor((p.K[many] - 1.0) * (N - p.L[many]) / (p.K[many] - 1.0) + 0.5)
        assert (last + p.L[many] <= N).all(), kw
    print(f"N={N}: worst f / fres / b difference {worst:.2f} ulp")
    assert worst <= 4.0


def test_emitted_bin_is_at_least_bmin():
    """`b >= bmin` on the emitted b over the whole grid. The plan loop alone (LTPDA's; the
    restatement with literal=True) does not keep it: b >= bmin holds for the bin chosen before
    L = floor(fs/fres + 0.5) is rounded, and b = f L / fs then moves by up to f / (2 fs) — 77
    of the 360 grid plans hold a frequency below bmin, the lowest b / bmin 0.9522 (N = 20000,
    Jdes 27, Kdes 1, bmin 2.5, olap 0: L = 9). The plan's bin floor lengthens such a segment to
    the shortest that keeps b >= bmin; a plan whose loop never drops below bmin is the loop's,
    entry for entry."""
    low, floored = [], 0
    for n, Jdes, Kdes, bmin, Lmin, olap in GRID:
        kw = dict(olap=olap, bmin=bmin, Lmin=Lmin, Jdes=Jdes, Kdes=Kdes)
        p = _plan(n, **kw)
        if p.f.size and (p.b < bmin).any():
            low.append((float((p.b / bmin).min()), n, Jdes, Kdes, bmin, Lmin, olap))
        lit = R.plan(n, FS, literal=True, **kw)
        if (lit[2] >= bmin).all():
            assert p.f.size == lit[0].size and np.array_equal(p.L, lit[3]) and np.array_equal(p.K, lit[4]), kw
            assert p.f.size == 0 or float(_ulps(p.f, lit[0]).max()) <= 4.0, kw
        else:
            floored += 1
    print(f"{len(low)} of {len(GRID)} plans hold b < bmin; {floored} plans use the bin floor")
    assert not low, min(low)
    assert floored == 77


def test_default_settings_give_the_documented_plans():
    p = _plan(500, Jdes=100)
    assert (p.f.size, p.L.min(), p.L.max(), p.K.min(), p.K.max()) == (27, 28, 500, 1, 73)
    p = _plan(10**7)
    assert p.f.size == 348
    assert abs(p.L.sum() / 1e7 - 11.0) < 0.05 and abs((p.L * p.K).sum() / 1e7 - 1450) < 1


def test_count_only_and_capacity():
    from deepfmkit_amd import _lib
    lib = _lib.load()
    a = (500, FS, 0.5, 1.0, 0, 100, 100)
    J = lib.dfmi_lpsd_plan(*a, None, None, None, None, None, 0)
    assert J == _plan(500, olap=0.5, Jdes=100).f.size
    f, fres, b = np.zeros(J), np.zeros(J), np.zeros(J)
    L, K = np.zeros(J, dtype=np.int64), np.zeros(J, dtype=np.int64)
    ptrs = [_lib.ptr(v) for v in (f, fres, b, L, K)]
    assert lib.dfmi_lpsd_plan(*a, *ptrs, J) == J
    assert lib.dfmi_lpsd_plan(*a, *ptrs, J - 1) == -1  # no room
    assert lib.dfmi_lpsd_plan(*a, ptrs[0], None, *ptrs[2:], J) == -1  # all five outputs or none


@pytest.mark.parametrize("bad", [dict(N=7), dict(fs=0.0), dict(fs=-1.0), dict(fs=float("nan")), dict(olap=-0.1),
                                 dict(olap=1.0), dict(olap=float("nan")), dict(bmin=0.0), dict(bmin=-1.0),
                                 dict(Jdes=0), dict(Kdes=0)])
def test_rejected_arguments(bad):
    from deepfmkit_amd import _lib
    lib = _lib.load()
    a = dict(N=500, fs=FS, olap=0.5, bmin=1.0, Lmin=0, Jdes=100, Kdes=100)
    a.update(bad)
    assert lib.dfmi_lpsd_plan(*a.values(), None, None, None, None, None, 0) == -1  # DFMI_ERR_ARG
    with pytest.raises(ValueError):
        _plan(a["N"], fs=a["fs"], olap=a["olap"], bmin=a["bmin"], Jdes=a["Jdes"], Kdes=a["Kdes"])
