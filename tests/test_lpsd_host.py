"""csrc/lpsd.h's point functions (what dfmi_lpsd's kernels run per lane) through their host
build tests/hostcheck_lpsd: the Kaiser window against np.kaiser, Sxx against the numpy
restatement at the shapes and gate of tests/test_gpu_lpsd.py (tests/helpers/lpsd_cases.py),
the sine known answer, and the white-noise sanity of the definition itself. CPU only.

Worst observed ratio to the gate (host build; DESIGN.md §13, profiles/lpsd/gate_ratios_host.txt):
0.153 (s1, mean -1, order 0), 0.142 (s2), 0.104 (s3); window within 2.6e-15 of np.kaiser."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lpsd_cases as C  # noqa: E402
import lpsd_ref as R  # noqa: E402

HC = os.path.join(os.path.dirname(__file__), "hostcheck_lpsd", "libhostcheck_lpsd.so")


@pytest.fixture(scope="module")
def hc():
    assert os.path.exists(HC), "tests/hostcheck_lpsd not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(HC)
    P, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    lib.hc_lpsd_alpha.argtypes = [dbl]
    lib.hc_lpsd_alpha.restype = dbl
    lib.hc_lpsd_window.argtypes = [i64, dbl, P, P]
    lib.hc_lpsd_window.restype = None
    lib.hc_lpsd_plan.argtypes = [i64, dbl, dbl, dbl, i64, i64, i64, P, P, P, P, P, i64]
    lib.hc_lpsd_plan.restype = i64
    lib.hc_lpsd.argtypes = [P, i64, i64, i64, dbl, P, P, P, i64, ctypes.c_int32, dbl, P, P]
    lib.hc_lpsd.restype = None
    return lib


def _run(hc, x, order=0, psll=200.0, **kw):
    x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
    f, fres, b, L, K = R.plan(x.shape[1], C.FS, psll=psll, **kw)
    Sxx, enbw = np.empty((x.shape[0], f.size)), np.empty(f.size)
    hc.hc_lpsd(x.ctypes.data, x.shape[0], x.shape[1], x.shape[1], C.FS, b.ctypes.data, L.ctypes.data, K.ctypes.data,
               f.size, order, psll, Sxx.ctypes.data, enbw.ctypes.data)
    return Sxx, enbw


def test_kaiser_constants(hc):
    from deepfmkit_amd import lpsd as M
    assert abs(hc.hc_lpsd_alpha(200.0) - 8.0858879) < 1e-12
    assert hc.hc_lpsd_alpha(200.0) == M.kaiser_alpha(200) == R.kaiser_alpha(200)
    assert abs(M.default_olap(200) - 0.7658465) < 5e-8
    assert M.default_olap(200) == R.default_olap(R.kaiser_alpha(200))


@pytest.mark.parametrize("L", [21, 64, 257, 4096])
def test_window_against_numpy_kaiser(hc, L):
    """w[n] = np.kaiser(L + 1, pi alpha)[:L]. Tolerance 1e-13 of the window's peak (1): the
    argument pi alpha sqrt(1 - z^2) carries ~3 roundings, 1 - z^2 cancels near the edges by up
    to L/4, and I0's sensitivity to its squared argument is I0'/(2x) <= I0/4 per unit, so
    either side is within (pi alpha)^2 / 4 * 3 * 2^-53 = 5.4e-14 of the true sample; np.i0's
    own Chebyshev error (Cephes: 5.8e-16 relative, twice for the ratio) is below that."""
    w, sums = np.empty(L), np.empty(2)
    hc.hc_lpsd_window(L, 200.0, w.ctypes.data, sums.ctypes.data)
    ref = np.kaiser(L + 1, np.pi * R.kaiser_alpha(200))[:L]
    err = float(np.abs(w - ref).max())
    print(f"L={L}: max |w - np.kaiser| = {err:.2e}")
    assert err <= 1e-13
    assert w[0] == w.min() and abs(w[L // 2] - 1.0) < (1e-13 if L % 2 == 0 else 0.05)
    assert abs(sums[0] - ref.sum()) <= 1e-13 * L and abs(sums[1] - (ref * ref).sum()) <= 1e-13 * L


def test_host_plan_is_the_library_plan(hc):
    from deepfmkit_amd import lpsd as M
    p = M.plan(4096, C.FS, Jdes=60)
    J = hc.hc_lpsd_plan(4096, C.FS, M.default_olap(200), 1.0, 0, 60, 100, None, None, None, None, None, 0)
    assert J == p.f.size
    f, fres, b = np.empty(J), np.empty(J), np.empty(J)
    L, K = np.empty(J, dtype=np.int64), np.empty(J, dtype=np.int64)
    assert hc.hc_lpsd_plan(4096, C.FS, M.default_olap(200), 1.0, 0, 60, 100, f.ctypes.data, fres.ctypes.data,
                           b.ctypes.data, L.ctypes.data, K.ctypes.data, J) == J
    assert np.array_equal(L, p.L) and np.array_equal(K, p.K)
    assert np.allclose(f, p.f, rtol=1e-15, atol=0) and np.allclose(b, p.b, rtol=1e-15, atol=0)


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_sxx_against_the_restatement(hc, shape):
    worst = 0.0
    for mean in C.MEANS:
        for order in C.ORDERS:
            x, _, enbw_ref, gate = C.reference(shape, mean, order)
            Sxx, enbw = _run(hc, x, order=order, **C.settings(shape))
            r = C.ratio(Sxx[0], shape, mean, order)
            print(f"{shape} mean {mean:g} order {order}: gate {gate:.2e} ratio {r:.3g}")
            worst = max(worst, r)
            assert np.max(np.abs(enbw / enbw_ref - 1)) <= 1e-12
    assert worst <= 1.0, worst


def test_sine_known_answer(hc):
    """Sxx ENBW = A^2/2 at a plan frequency with b >= 9, within 1e-9 relative."""
    j = C.KNOWN["js"][1]
    Sxx, enbw = _run(hc, C.known_series(j), Jdes=C.KNOWN["Jdes"])
    rel = Sxx[0, j] * enbw[j] / (C.KNOWN["amp"] ** 2 / 2) - 1
    print(f"j={j}: Sxx ENBW / (A^2/2) - 1 = {rel:.2e}")
    assert abs(rel) <= C.KNOWN["tol"]


def test_white_noise_level_of_the_definition(hc):
    """The definition itself on white noise of variance s^2: Sxx scatters about 2 s^2 / fs."""
    x = 1e-3 * np.random.RandomState(0).randn(20000)
    r = R.lpsd(x, C.FS, Jdes=100)
    med = float(np.median(r["Sxx"] / (2 * 1e-6 / C.FS)))
    print(f"restatement: median Sxx / (2 s^2 / fs) = {med:.4f}")
    assert 0.9 <= med <= 1.1
    Sxx, _ = _run(hc, x, Jdes=100)
    assert 0.9 <= float(np.median(Sxx[0] / (2 * 1e-6 / C.FS))) <= 1.1
    assert np.max(np.abs(Sxx[0] / r["Sxx"] - 1)) <= 1e-12
