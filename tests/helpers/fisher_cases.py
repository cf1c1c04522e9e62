"""Shared cases, numpy reference and gates of the dfmi_fisher tests (tests/test_fisher_*.py,
tests/test_gpu_fisher.py, tests/test_gpu_fit_errors.py).

Reference at arbitrary points: oracle.nls_oracle.model_and_jacobian for J^T J, np.linalg.inv
for the covariance (tests/test_fisher_golden.py shows it reproduces the fixture fisher.npz,
which the reference's own helpers.py / fit.coeffs wrote).

Gates (A, cov: the REFERENCE's matrices):
  J^T J   |dA_ij| <= 1e-13 sqrt(A_ii A_jj). No inverse, no amplification: an entry is a
          weighted sum of products of two device Bessel values, each within 3e-15 absolute
          (tests/test_gpu_numerics.py), with 4x margin.
  sigma   relative error <= 1e-13 (1 + cond_2(A)).
  cov     |dcov_ij| <= 1e-13 (1 + cond_2(A)) sqrt(cov_ii cov_jj): the relative error on the
          diagonal. The psi column is analytically orthogonal to the other three (a03, a13,
          a23 are zero in exact arithmetic), so cov_03, cov_13, cov_23 are rounding noise in
          the reference as well and an entry-wise relative error has no meaning for them
          (about 4e14 on the fixture's random points): off-diagonal entries are measured on
          the scale of their two variances, as J^T J is.
  The reference's own fp64 inverse moves by up to 0.11 eps cond against an extended-precision
  inverse; the gate is 1.4e-11 at the grids' median cond of 140 and loose only where the
  reference's answer is itself that uncertain (cond 3.7e8 at m = 0.1).
Every check returns the worst observed ratio to its gate (<= 1 passes)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import nls_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fisher.npz")
UPPER = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
GATE = 1e-13


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def snr_var(snr_db):
    """calculate_m_precision's variance factor (helpers.py:117-118)."""
    return (1.0 / 10 ** (snr_db / 20.0)) ** 2


def crlb_var(snr_db, buffer_size):
    """calculate_crlb_for_m's variance factor (helpers.py:23-28)."""
    return (0.5 / 10 ** (snr_db / 10.0)) / (2 * buffer_size)


def mprec_points(m):
    """calculate_m_precision's points (helpers.py:116): (1, m, pi/4, 0), component-major."""
    p = np.zeros((4, len(m)))
    p[0], p[1], p[2] = 1.0, m, np.pi / 4
    return p


def reference(p, ndata):
    """numpy reference at points p (4, n), ndata scalar or (n,):
    A (n, 4, 4), inv(A) (n, 4, 4) (NaN where numpy refuses), cond_2(A) (n,)."""
    p = np.asarray(p, dtype=np.float64)
    n = p.shape[1]
    nd = np.broadcast_to(np.asarray(ndata), (n,))
    A = np.empty((n, 4, 4))
    X = np.full((n, 4, 4), np.nan)
    cond = np.full(n, np.inf)
    for s in range(n):
        k = int(nd[s])
        A[s] = O.model_and_jacobian(k, np.zeros(2 * k), p[:, s])[1].reshape(4, 4)
        if np.isfinite(A[s]).all():
            try:
                X[s] = np.linalg.inv(A[s])
                cond[s] = np.linalg.cond(A[s])
            except np.linalg.LinAlgError:
                pass
    return A, X, cond


def upper(M):
    """(n, 4, 4) -> (10, n) in dfmi_fisher's order."""
    return np.array([M[:, r, c] for r, c in UPPER])


def ratio_jtj(jtj, A):
    """Worst |dA_ij| / (GATE sqrt(A_ii A_jj)) of a (10, n) result against A (n, 4, 4)."""
    d = np.sqrt(np.einsum("nii->ni", A))
    scale = np.array([d[:, r] * d[:, c] for r, c in UPPER])
    return float((np.abs(jtj - upper(A)) / (GATE * scale)).max())


def ratio_sigma(sigma, X, cond, var=1.0):
    """Worst relative error of a (4, n) sigma against sqrt(var diag(X)), over its gate."""
    ref = np.sqrt(np.einsum("nii->in", X) * var)
    return float((np.abs(sigma - ref) / ref / (GATE * (1.0 + cond))).max())


def ratio_cov(cov, X, cond, var=1.0):
    """Worst |dcov_ij| / (gate sqrt(cov_ii cov_jj)) of a (10, n) cov against var X."""
    C = X * np.reshape(var * np.ones(X.shape[0]), (-1, 1, 1))
    d = np.sqrt(np.einsum("nii->ni", C))
    scale = np.array([d[:, r] * d[:, c] for r, c in UPPER])
    return float((np.abs(cov - upper(C)) / scale / (GATE * (1.0 + cond))).max())


@functools.lru_cache(maxsize=None)
def grid_cases():
    """The fixture's calculate_m_precision grids: [(name, params (4, n), ndata, var, expected
    delta_m (n,) from the fixture, (A, X, cond) numpy reference)], computed once."""
    g = golden()
    out = []
    for i, nd in enumerate(g["mprec_nd80"]):
        p = mprec_points(g["mprec_m80"])
        out.append((f"m80_nd{int(nd)}", p, int(nd), snr_var(80.0), g["mprec_80"][i], reference(p, int(nd))))
    p = mprec_points(g["mprec_m10"])
    ref10 = reference(p, 10)
    for i, snr in enumerate(g["mprec_snr10"]):
        out.append((f"nd10_snr{int(snr)}", p, 10, snr_var(float(snr)), g["mprec_10"][i], ref10))
    return out


@functools.lru_cache(maxsize=None)
def random_cases():
    """The fixture's random points grouped by ndata: [(ndata, index array, params (4, k),
    (A, X, cond))] (dfmi_fisher takes one ndata per call)."""
    g = golden()
    out = []
    for nd in np.unique(g["rnd_nd"]):
        idx = np.where(g["rnd_nd"] == nd)[0]
        p = np.ascontiguousarray(g["rnd_p"][idx].T)
        out.append((int(nd), idx, p, reference(p, int(nd))))
    return out


# points without an inverse: amp = 0 (column 0 and, through a, every other column vanish),
# m = 0 (J_j(0) = 0, j >= 1: column 0 and the phi, psi columns vanish), a NaN parameter
SINGULAR = np.array([[0.0, 6.0, 0.3, 0.1], [1.2, 0.0, 0.3, 0.1], [1.0, np.nan, 0.3, 0.1],
                     [0.0, 0.0, 0.0, 0.0], [1.0, 6.0, np.nan, 0.0]]).T
REGULAR = np.array([[1.0, 6.0, 0.3, 0.1], [1.6, -7.5, 2.0, -0.4]]).T


def check_singular(ok, sigma, cov, jtj):
    """dfmi_fisher at SINGULAR: ok = 0, NaN cov and sigma, J^T J as computed."""
    assert (np.asarray(ok) == 0).all(), ok
    assert np.isnan(sigma).all() and np.isnan(cov).all()
    assert (jtj[:, 0] == 0.0).all() and (jtj[:, 3] == 0.0).all()  # amp = 0: every column is zero
    assert jtj[0, 1] == 0.0 and jtj[7, 1] == 0.0 and jtj[9, 1] == 0.0 and jtj[4, 1] > 0.0  # m = 0: d/dm stays
    assert np.isnan(jtj[:, 2]).all() and np.isnan(jtj[:, 4]).any()


# ---- the statistical record (tests/test_fisher_host.py, tests/test_gpu_fit_errors.py) ----
STAT = dict(f_samp=200000.0, f_mod=1000.0, n=1, R=200, nbuf=2000, ndata=10, snr_db=40.0,
            truth=(1.0, 6.0, 0.7, 0.3))
STAT_BAND = 5.0 / np.sqrt(2.0 * (STAT["nbuf"] - 1))  # five standard errors of an empirical std: 0.079


@functools.lru_cache(maxsize=None)
def stat_record():
    """y = 1 + cos(0.7 + 6 cos(2 pi 1000 t + 0.3)) + white noise at 40 dB (a unit cosine has
    power 0.5: std sqrt(0.5 / 1e4)) from RandomState(1); 2,000 buffers of R = 200."""
    N = STAT["R"] * STAT["nbuf"]
    t = np.arange(N) / STAT["f_samp"]
    y = 1.0 + np.cos(0.7 + 6.0 * np.cos(2 * np.pi * STAT["f_mod"] * t + 0.3))
    y += np.random.RandomState(1).normal(0.0, np.sqrt(0.5 / 10 ** (STAT["snr_db"] / 10.0)), N)
    y.setflags(write=False)
    return y


def stat_ratios(fitted, err):
    """sqrt(mean(err^2)) / std(fitted, ddof=1) per parameter; fitted, err: (4, nbuf)."""
    return np.sqrt((np.asarray(err) ** 2).mean(axis=1)) / np.asarray(fitted).std(axis=1, ddof=1)
