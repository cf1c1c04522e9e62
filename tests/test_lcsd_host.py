"""csrc/lpsd.h's pair forms (what dfmi_lcsd's kernels run per lane) through their host build
tests/hostcheck_lcsd: Sxx, Syy, Sxy and the coherence against the numpy restatement at the
shapes and gates of tests/test_gpu_lcsd.py (tests/helpers/lcsd_cases.py), Sxx and Syy bit for bit
the host build of the single-series path, the two-sine known answer and the white-noise
statistics of the definition. CPU only.

Worst observed ratio to the gate (host build; DESIGN.md §15, profiles/lcsd/gate_ratios_host.txt):
Sxx 0.153 (s1), Syy 0.0625 (s3), Sxy 0.0737 (s2), coh 0.0662 (s2), each at mean -1, order 0; the
known answer 1.29e-12 (Sxy), 6.6e-14 (H), 2.3e-16 (coh) against the bound 1e-9; statistics: median
coh 0.0023 (independent), 0.486, |H| 0.986, resid 0.980 (x against x + n)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lcsd_cases as C  # noqa: E402
import lcsd_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HC = os.path.join(HERE, "hostcheck_lcsd", "libhostcheck_lcsd.so")
HC_LPSD = os.path.join(HERE, "hostcheck_lpsd", "libhostcheck_lpsd.so")
P, i64, dbl, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_int32


@pytest.fixture(scope="module")
def hc():
    assert os.path.exists(HC), "tests/hostcheck_lcsd not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(HC)
    lib.hc_lcsd.argtypes = [P, i64, P, i64, i64, i64, dbl, P, P, P, i64, i32, dbl, P, P, P, P, P, P]
    lib.hc_lcsd.restype = None
    return lib


@pytest.fixture(scope="module")
def hc_lpsd():
    assert os.path.exists(HC_LPSD), "tests/hostcheck_lpsd not built (run __graft_entry__.build())"
    lib = ctypes.CDLL(HC_LPSD)
    lib.hc_lpsd.argtypes = [P, i64, i64, i64, dbl, P, P, P, i64, i32, dbl, P, P]
    lib.hc_lpsd.restype = None
    return lib


def _run(hc, x, y, order=0, psll=200.0, **kw):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    f, fres, b, L, K = R.plan(x.size, C.FS, psll=psll, **kw)
    o = [np.empty(f.size) for _ in range(6)]
    hc.hc_lcsd(x.ctypes.data, 0, y.ctypes.data, 0, 1, x.size, C.FS, b.ctypes.data, L.ctypes.data, K.ctypes.data, f.size,
               order, psll, *(a.ctypes.data for a in o))
    Sxy = o[2] + 1j * o[3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(Sxx=o[0], Syy=o[1], Sxy=Sxy, coh=o[4], enbw=o[5], H=Sxy / o[0], resid=o[1] * (1 - o[4]), K=K)


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_against_the_restatement(hc, hc_lpsd, shape):
    worst = dict.fromkeys(C.QUANTITIES, 0.0)
    for mean in C.MEANS:
        for order in C.ORDERS:
            x, y, ref, gates = C.reference(shape, mean, order)
            r = _run(hc, x, y, order=order, **C.settings(shape))
            rat = C.ratios(r, shape, mean, order)
            print(f"{shape} mean {mean:g} order {order}: " +
                  ", ".join(f"{q} gate {gates[q]:.2e} ratio {rat[q]:.3g}" for q in C.QUANTITIES))
            worst = {q: max(worst[q], rat[q]) for q in C.QUANTITIES}
            assert np.max(np.abs(r["enbw"] / ref["enbw"].astype(np.float64) - 1)) <= 1e-12
            # the pair form did not drift from the single-series path: the same bits
            f, _, b, L, K = R.plan(x.size, C.FS, **C.settings(shape))
            both = np.stack([x, y])
            S, enbw = np.empty((2, f.size)), np.empty(f.size)
            hc_lpsd.hc_lpsd(both.ctypes.data, 2, x.size, x.size, C.FS, b.ctypes.data, L.ctypes.data, K.ctypes.data, f.size,
                            order, 200.0, S.ctypes.data, enbw.ctypes.data)
            assert np.array_equal(S[0], r["Sxx"]) and np.array_equal(S[1], r["Syy"]) and np.array_equal(enbw, r["enbw"])
    print(f"{shape}: worst ratio to the gate " + ", ".join(f"{q} {worst[q]:.3g}" for q in C.QUANTITIES))
    assert max(worst.values()) <= 1.0, worst


def test_restatement_sxx_is_the_single_series_restatement():
    import lpsd_ref
    x, y = C.pair("s2", -1.0)
    r = R.lcsd(x, y, C.FS, **C.settings("s2"))
    assert np.array_equal(r["Sxx"], lpsd_ref.lpsd(x, C.FS, **C.settings("s2"))["Sxx"])
    assert np.array_equal(r["Syy"], lpsd_ref.lpsd(y, C.FS, **C.settings("s2"))["Sxx"])


def test_two_sine_known_answer(hc):
    """Sxy ENBW = Ax Ay / 2 e^{-i lag}, H = Ay / Ax e^{-i lag}, coh = 1, each within 1e-9."""
    for j in C.KNOWN["js"]:
        x, y = C.known_pair(j)
        r = _run(hc, x, y, Jdes=C.KNOWN["Jdes"])
        fig = C.check_known(r["Sxy"], r["H"], r["coh"], r["enbw"], j)
        print(f"j={j}: |Sxy ENBW / expected - 1| = {fig[0]:.2e}, |H - expected| = {fig[1]:.2e}, |coh - 1| = {fig[2]:.2e}")
        assert max(fig) <= C.KNOWN["tol"]


def test_white_noise_statistics(hc):
    x, n = C.stat_series()
    a = _run(hc, x, n, Jdes=C.STAT["Jdes"])
    s = _run(hc, x, x + n, Jdes=C.STAT["Jdes"])
    C.check_statistics((a["coh"], a["H"], a["resid"]), (s["coh"], s["H"], s["resid"]), a["K"])


def test_npair_strides_shared_x_and_null_outputs(hc):
    """The host build's call geometry: rows at a stride, x_stride 0, outputs left out."""
    kw = C.settings("s1")
    x, y = C.pair("s1", -1.0)
    one = _run(hc, x, y, **kw)
    f, _, b, L, K = R.plan(x.size, C.FS, **kw)
    ys = np.full((3, x.size + 13), np.nan)
    ys[:, :x.size] = np.stack([y, x, 2 * y])
    coh, re = np.empty((3, f.size)), np.empty((3, f.size))
    hc.hc_lcsd(x.ctypes.data, 0, ys.ctypes.data, x.size + 13, 3, x.size, C.FS, b.ctypes.data, L.ctypes.data,
               K.ctypes.data, f.size, 0, 200.0, None, None, re.ctypes.data, None, coh.ctypes.data, None)
    assert np.array_equal(coh[0], one["coh"]) and np.array_equal(re[0], one["Sxy"].real)
    assert np.max(np.abs(coh[1] - 1)) <= 1e-12   # x against itself
    assert np.array_equal(re[2], 2 * re[0])       # a power of two scales exactly
