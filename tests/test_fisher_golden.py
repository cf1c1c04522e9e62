"""The numpy reference of the dfmi_fisher tests (tests/helpers/fisher_cases.py: the oracle's
model_and_jacobian + np.linalg.inv) reproduces the fixture fisher.npz, which the reference's
helpers.py (calculate_m_precision, calculate_crlb_for_m, calculate_jacobian) and fit.coeffs
wrote (tests/golden/make_fisher_golden.py). CPU only; at the gates of fisher_cases."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import fisher_cases as C  # noqa: E402


def test_fixture_is_small_and_complete():
    assert os.path.getsize(C.GOLDEN) < 150 * 1024
    g = C.golden()
    assert g["mprec_80"].shape == (9, 500) and g["mprec_10"].shape == (3, 500)
    assert g["rnd_p"].shape == (300, 4) and g["rnd_nd"].min() == 3 and g["rnd_nd"].max() == 62
    assert (np.abs(g["rnd_p"][:, 1]) >= 64).sum() >= 8 and (g["rnd_p"][:, 1] < 0).sum() > 100
    assert all(np.isfinite(g[k]).all() for k in ("mprec_80", "mprec_10", "crlb", "rnd_sig"))  # 0 non-finite


def test_oracle_jtj_and_inverse_reproduce_the_reference_coeffs_points():
    g = C.golden()
    worst_a = worst_s = 0.0
    for nd, idx, p, (A, X, cond) in C.random_cases():
        worst_a = max(worst_a, C.ratio_jtj(g["rnd_jtj"][idx].T, A))
        worst_s = max(worst_s, C.ratio_sigma(g["rnd_sig"][idx].T, X, cond))
    print(f"oracle vs fit.coeffs: jtj ratio {worst_a:.3g}, sigma ratio {worst_s:.3g}")
    assert worst_a <= 1.0 and worst_s <= 1.0


def test_oracle_reproduces_calculate_m_precision_grids():
    worst = 0.0
    for name, p, nd, var, expect, (A, X, cond) in C.grid_cases():
        assert np.isfinite(X).all(), name  # the reference inverts every grid point
        ref = np.sqrt(var * X[:, 1, 1])
        worst = max(worst, float((np.abs(ref - expect) / expect / (C.GATE * (1 + cond))).max()))
    print(f"oracle vs calculate_m_precision: ratio {worst:.3g}")
    assert worst <= 1.0


def test_oracle_reproduces_calculate_crlb_and_jacobian():
    g = C.golden()
    worst = 0.0
    for (m, nd, snr, R), expect in zip(g["crlb_args"], g["crlb"]):
        A, X, cond = C.reference(np.array([[1.0], [m], [0.0], [0.0]]), int(nd))
        ref = np.sqrt(X[0, 1, 1] * C.crlb_var(snr, R))
        worst = max(worst, abs(ref - expect) / expect / (C.GATE * (1 + cond[0])))
    assert worst <= 1.0, worst
    for p, nd, J in zip(g["jac_p"], g["jac_nd"], g["jac"]):
        A = C.reference(p.reshape(4, 1), int(nd))[0]
        JtJ = J.T @ J
        if p[0] == 0.0:
            assert (JtJ == 0).all() and (A == 0).all()
        else:
            assert C.ratio_jtj(C.upper(JtJ[None]), A) <= 1.0
