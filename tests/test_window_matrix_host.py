"""CPU validation of the window matrix's reference and inputs (tests/helpers/window_ref.py), so that
the GPU tests (tests/test_gpu_window_matrix.py, tests/test_gpu_window_records.py) cannot hide behind
them: the long-double definition against a sample-by-sample evaluation and against the numpy oracle's
rectangular demodulation, the window's sum, the record set's oracle statuses and their stability, and
the instance table against the dispatch rules of demod_window_device.

Bound of the brute-force comparison: both sides round every term to long double (eps = 1.08e-19); the
window angle is below 2 pi K <= 19 unreduced and the basis angle below ndata w0 R <= 150 at the shapes
used, so a term is off by at most ~150 eps max|x|, and a mean of R <= 403 terms, summed in sequence on
one side and pairwise on the other, by at most R eps max|x| more: (403 + 150) x 1.08e-19 = 6.0e-17 <
1e-16. The QI error is taken against max|x| (a harmonic may vanish), dc relative."""
import os
import sys

import numpy as np
import pytest

from conftest import compare_fit, record_tol

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import window_ref as W  # noqa: E402

from oracle import nls_oracle as O  # noqa: E402

BRUTE = [(403, 200, "hann", 3), (130, 200, "blackmanharris", 2), (4, 200, "blackmanharris", 2), (378, 75, "blackman", 4),
         (15, 2, "hamming", 3), (200, 200, "hann", 2)]


def test_long_double_is_extended():
    assert np.finfo(np.longdouble).eps < 1.1e-19, "np.longdouble is no wider than float64 here: no reference"


@pytest.mark.parametrize("R,L,window,nd", BRUTE)
def test_reference_against_sample_by_sample(R, L, window, nd):
    w0 = 2 * np.pi / L
    for dtype in ("float64", "int16"):
        seg = W.signal(R, w0, dtype, seed=R)
        qi, dc = W.reference(seg[None, :], window, nd, w0)
        bq, bd = W.brute(seg, window, nd, w0)
        eq = float(np.abs(qi[:, 0] - bq).max() / np.abs(seg.astype(np.longdouble)).max())
        ed = float(abs((dc[0] - bd) / bd))
        print(f"R={R} L={L} {window} {dtype}: QI {eq:.2e} of max|x|, dc {ed:.2e} relative")
        assert eq <= 1e-16 and ed <= 1e-16


@pytest.mark.parametrize("window", ["hann", "hamming", "blackman", "blackmanharris", [0.3, 0.2, -0.1, 0.05]])
def test_window_sum_is_R_a0(window):
    a = W.coefs(window)
    for R in (len(a), len(a) + 1, 7, 130, 800, 1003, 2003):  # R > K = len(a) - 1
        s = W.weights(R, window).sum()
        assert abs(s - np.longdouble(R) * np.longdouble(a[0])) <= 1e-17 * R, (R, s)


def test_one_coefficient_is_the_oracle_demodulation():
    for R, L, nd in ((1003, 200, 10), (378, 75, 7), (800, 200, 10)):
        w0 = 2 * np.pi / L
        seg = W.signal(R, w0, seed=3)
        qi, dc = W.reference(seg[None, :], [1.0], nd, w0)
        ref = O.demod_buffer(seg, nd, w0)
        assert np.abs(qi[:, 0] - ref).max() <= 1e-13 * np.abs(seg).max()
        assert abs(dc[0] - seg.mean()) <= 1e-13 * seg.mean()


def test_instance_table():
    rows = W.INSTANCES
    keys = {(r["vec"], r["ms"], r["K"], r["dtype"]) for r in rows}
    assert len(rows) == 36 and len(keys) == 36
    assert keys == {(v, m, k, d) for v in (1, 2) for m in (2, 4) for k in (1, 2, 3) for d in W.DTYPES}
    for r in rows:
        assert r["R"] == 5 * r["L"] + 3 and r["stride"] >= r["R"]
        assert W.expected_instance(r["L"], r["stride"]) == (r["vec"], r["ms"]), r
        assert len(W.coefs(r["window"])) - 1 == r["K"]
        assert r["R"] // r["L"] == 5 and r["R"] % r["L"] == 3  # UNR 4: 4 + 1 cycles; UNR 2: 2 + 2 + 1; ragged 3
        x, _ = W.instance_input(r)
        assert x.dtype == np.dtype(r["dtype"]) and x.size == (W.NSEG - 1) * r["stride"] + r["R"] and x.min() > 0
    # the same rules where a device view starts one sample in, and at the matrix's other shapes
    assert W.expected_instance(200, 1004, base_aligned=False) == (1, 4)
    assert W.expected_instance(128, 644) == (2, 2) and W.expected_instance(512, 2048) == (2, 4)
    assert W.expected_instance(400, 1004) == (2, 4) and W.expected_instance(2, 15) == (1, 2)


def _cases():
    return [(ds, dt, w, m) for ds in W.DATASETS for dt in W.DTYPES for w in W.WINDOWS for m in W.MODES
            if dt == "float64" or (ds == "rec800" and m is None)]


@pytest.mark.parametrize("dataset,dtype,window,mode", _cases())
def test_record_set_statuses(dataset, dtype, window, mode):
    """Every oracle status is 0, and stays 0 with the fits inside the gate when every QI value moves
    by 1e-15 relative (tests/test_record_matrix_host.py's check). If a record fails this, change the
    record in window_ref, not the gate."""
    ref = W.oracle(dataset, dtype, window, mode)
    assert (ref["fitok"] == 0).all(), np.where(ref["fitok"] != 0)
    qi = ref["qi"]
    sign = np.random.RandomState(91).choice([-1.0, 1.0], qi.shape)
    again = W.oracle(dataset, dtype, window, mode, qi=qi * (1.0 + 1e-15 * sign))
    np.testing.assert_array_equal(again["fitok"], ref["fitok"])
    compare_fit(again, ref, tol=record_tol(W.ND, qi, ref), min_status_match=1.0)


def test_record_set_shape():
    x, g = W.records(), W.guesses()
    assert x.shape == (W.NREC, W.NBUF * W.R) and W.NREC > 8 and W.R // 200 > 3 and x.min() > 0
    assert W.long_record().shape == ((W.NREC - 1) * W.NBUF * W.HOP + (W.NBUF - 1) * W.HOP + W.R,)
    assert len({tuple(r) for r in g}) == W.NREC and np.allclose(np.abs(g[:, 1] - np.linspace(5, 7, 9)), 0.4)
    assert np.abs(W.records("int16")).max() <= 20000 and np.abs(W.long_record("int16")).max() <= 20000
    np.testing.assert_array_equal(W.segments("long400")[W.NBUF], W.long_record()[2800:3600])
    np.testing.assert_array_equal(W.segments("rec400")[W.NBUF + 1], x[1, 400:1200])
