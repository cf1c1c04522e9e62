"""csrc/fisher.h's point function (what dfmi_fisher's kernel runs per lane) through its host
build tests/hostcheck_fisher, at the gates of tests/helpers/fisher_cases.py: the fixture's
calculate_m_precision grids, its random points (J^T J, cov, sigma), the points without an
inverse; and the oracle-only form of the statistical check of tests/test_gpu_fit_errors.py
(the chosen record sits inside its band). CPU only; the GPU twin is tests/test_gpu_fisher.py.

Worst observed ratios to the gates (host build): J^T J 0.115, sigma 0.0023,
cov 0.0046 (the fixture's random points); the oracle's statistical ratios 0.992 - 1.006."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fisher_cases as C  # noqa: E402

HC = os.path.join(os.path.dirname(__file__), "hostcheck_fisher", "libhostcheck_fisher.so")


@pytest.fixture(scope="module")
def hc():
    assert os.path.exists(HC), "tests/hostcheck_fisher not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(HC)
    P = ctypes.c_void_p
    lib.hc_fisher.argtypes = [P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, P, ctypes.c_double, P, P, P, P]
    lib.hc_fisher.restype = None

    def run(p, ndata, var=None, var_mul=1.0):
        p = np.ascontiguousarray(p, dtype=np.float64)
        n = p.shape[1]
        jtj, cov, sig = np.empty((10, n)), np.empty((10, n)), np.empty((4, n))
        ok = np.empty(n, dtype=np.int32)
        v = None if var is None else np.ascontiguousarray(var, dtype=np.float64)
        lib.hc_fisher(p.ctypes.data, n, n, ndata, None if v is None else v.ctypes.data, var_mul, jtj.ctypes.data,
                      cov.ctypes.data, sig.ctypes.data, ok.ctypes.data)
        return jtj, cov, sig, ok
    return run


def test_m_precision_grids(hc):
    wa = ws = wc = wf = 0.0
    for name, p, nd, var, expect, (A, X, cond) in C.grid_cases():
        jtj, cov, sig, ok = hc(p, nd, var_mul=var)
        assert (ok == 1).all(), name
        wa = max(wa, C.ratio_jtj(jtj, A))
        ws = max(ws, C.ratio_sigma(sig, X, cond, var))
        wc = max(wc, C.ratio_cov(cov, X, cond, var))
        wf = max(wf, float((np.abs(sig[1] - expect) / expect / (C.GATE * (1 + cond))).max()))  # the fixture itself
    print(f"host grids: jtj {wa:.3g} sigma {ws:.3g} cov {wc:.3g} delta_m vs fixture {wf:.3g}")
    assert max(wa, ws, wc, wf) <= 1.0, (wa, ws, wc, wf)


def test_random_points_with_per_point_variance(hc):
    wa = ws = wc = 0.0
    for nd, idx, p, (A, X, cond) in C.random_cases():
        var = 0.5 + (idx % 7)  # per point, times var_mul
        jtj, cov, sig, ok = hc(p, nd, var=var, var_mul=1e-4)
        assert (ok == 1).all(), nd
        wa = max(wa, C.ratio_jtj(jtj, A))
        ws = max(ws, C.ratio_sigma(sig, X, cond, var * 1e-4))
        wc = max(wc, C.ratio_cov(cov, X, cond, var * 1e-4))
    print(f"host random points: jtj {wa:.3g} sigma {ws:.3g} cov {wc:.3g}")
    assert max(wa, ws, wc) <= 1.0, (wa, ws, wc)


@pytest.mark.parametrize("ndata", [3, 10, 17, 62])
def test_points_without_an_inverse(hc, ndata):
    jtj, cov, sig, ok = hc(C.SINGULAR, ndata)
    C.check_singular(ok, sig, cov, jtj)
    # a non-finite or negative variance is not ok either; its neighbours are untouched, and a
    # zero variance is a valid one (sigma = 0)
    p = np.concatenate([C.REGULAR, C.REGULAR, C.REGULAR], axis=1)
    jtj, cov, sig, ok = hc(p, ndata, var=np.array([1.0, np.inf, np.nan, 2.0, -1e-3, 0.0]))
    assert list(ok) == [1, 0, 0, 1, 0, 1] and np.isnan(sig[:, [1, 2, 4]]).all() and np.isnan(cov[:, [1, 2, 4]]).all()
    assert np.isfinite(sig[:, [0, 3, 5]]).all() and (sig[:, 5] == 0).all() and (sig[:, [0, 3]] > 0).all()
    assert np.isfinite(jtj).all() and (jtj[:, :2] == jtj[:, 2:4]).all() and (jtj[:, :2] == jtj[:, 4:]).all()
    # the sign of var_mul counts too: the factor is var * var_mul
    assert list(hc(C.REGULAR, ndata, var=np.array([1.0, -1.0]), var_mul=-1.0)[3]) == [0, 1]


def test_statistical_band_with_the_oracle():
    """sqrt(mean sigma^2) / std(fitted) within 1 +- 5/sqrt(2 (2000 - 1)) = 1 +- 0.079 for amp, m,
    phi, psi on the 40 dB record, the numpy oracle fitting and numpy inverting. This runs none
    of the product's code: it shows that the record chosen for the GPU test
    (tests/test_gpu_fit_errors.py) sits inside the band, so a failure there is the product's."""
    from oracle import nls_oracle as O
    S = C.STAT
    fit = O.fit_record_parallel(C.stat_record(), S["f_samp"], S["f_mod"], S["n"], ndata=S["ndata"], n_cores=1)
    assert (fit[:, 6] == 0).all()
    p = np.ascontiguousarray(fit[:, :4].T)
    A, X, cond = C.reference(p, S["ndata"])
    err = np.sqrt(np.einsum("nii->in", X) * fit[:, 5] / (2 * S["ndata"] - 4))
    r = C.stat_ratios(p, err)
    print("oracle ratios sqrt(mean err^2)/std(fitted): amp %.4f m %.4f phi %.4f psi %.4f" % tuple(r))
    assert (np.abs(r - 1.0) <= C.STAT_BAND).all(), r
