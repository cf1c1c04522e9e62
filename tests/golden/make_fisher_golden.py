"""Fisher / CRLB fixtures from the reference DeepFMKit's helpers.py and fit.coeffs (run where
the reference is available only; the tests read fisher.npz alone).

  mprec_m80, mprec_nd80, mprec_80     calculate_m_precision(linspace(0.1, 30, 500), ndata, 80 dB)
                                      for ndata 3, 4, 8, 10, 12, 13, 16, 17, 30
  mprec_m10, mprec_snr10, mprec_10    calculate_m_precision(linspace(1, 30, 500), 10, snr) for
                                      20, 60, 100 dB (notebook 1.0_CRLB-bounds' grids)
  crlb_args (m, ndata, snr, R), crlb  calculate_crlb_for_m over a small table
  jac_p, jac_nd, jac                  calculate_jacobian at 20 points (a = 0, m < 0, ndata 62
                                      among them), rows beyond 2*ndata zero
  asd_args (snr, f_samp), asd         snr_to_asd
  rnd_p, rnd_nd, rnd_jtj, rnd_sig     fit.coeffs' J^T J (upper triangle, dfmi_fisher's order)
                                      and sqrt(diag(np.linalg.inv(J^T J))) at 300 seeded
                                      random points

Usage:  python tests/golden/make_fisher_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

UPPER = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))


def random_points(rng, n=300):
    p = np.empty((n, 4))
    p[:, 0] = rng.uniform(0.1, 3.0, n)
    p[:, 1] = rng.uniform(-40.0, 40.0, n)
    p[:, 2] = rng.uniform(-2 * np.pi, 2 * np.pi, n)
    p[:, 3] = rng.uniform(-np.pi, np.pi, n)
    nd = rng.randint(3, 63, n)
    # the large-argument Bessel branch: |m| in [64, 200] at ndata <= 16, both signs
    big = np.arange(0, n, 25)
    p[big, 1] = rng.uniform(64.0, 200.0, big.size) * np.where(np.arange(big.size) % 2, -1.0, 1.0)
    nd[big] = rng.randint(3, 17, big.size)
    return p, nd


def main():
    _, rfit, _ = _import_reference()
    import DeepFMKit.helpers as H
    out = {}
    m80 = np.linspace(0.1, 30, 500)
    nd80 = np.array([3, 4, 8, 10, 12, 13, 16, 17, 30])
    out["mprec_m80"], out["mprec_nd80"] = m80, nd80
    out["mprec_80"] = np.array([H.calculate_m_precision(m80, int(nd), 80.0) for nd in nd80])
    m10 = np.linspace(1, 30, 500)
    snr10 = np.array([20.0, 60.0, 100.0])
    out["mprec_m10"], out["mprec_snr10"] = m10, snr10
    out["mprec_10"] = np.array([H.calculate_m_precision(m10, 10, float(s)) for s in snr10])
    args = np.array([(m, nd, snr, R) for m in (0.5, 3.0, 6.0, 15.5, 29.0) for nd in (5, 10, 20)
                     for snr, R in ((20.0, 200), (60.0, 4000))], dtype=np.float64)
    out["crlb_args"] = args
    out["crlb"] = np.array([H.calculate_crlb_for_m(a[0], int(a[1]), a[2], int(a[3])) for a in args])
    rng = np.random.RandomState(20240607)
    jp = np.column_stack([rng.uniform(0.1, 3.0, 20), rng.uniform(0.1, 30.0, 20), rng.uniform(-7.0, 7.0, 20),
                          rng.uniform(-3.0, 3.0, 20)])
    jnd = rng.randint(3, 41, 20)
    jp[0, 0] = 0.0
    jp[1, 1], jp[2, 1] = -6.0, -0.3
    jnd[3], jnd[4] = 62, 62
    jp[5] = (1.0, 6.0, 0.0, 0.0)
    jac = np.zeros((20, 2 * 62, 4))
    for i in range(20):
        jac[i, :2 * jnd[i]] = H.calculate_jacobian(int(jnd[i]), jp[i])
    out["jac_p"], out["jac_nd"], out["jac"] = jp, jnd, jac
    asd_args = np.array([(s, f) for s in (0.0, 20.0, 40.0, 83.5, 120.0) for f in (30000.0, 200000.0, 1e6)])
    out["asd_args"] = asd_args
    out["asd"] = np.array([H.snr_to_asd(a[0], a[1]) for a in asd_args])
    p, nd = random_points(np.random.RandomState(7))
    jtj = np.empty((p.shape[0], 10))
    sig = np.empty((p.shape[0], 4))
    for i in range(p.shape[0]):
        _, flat, _ = rfit.coeffs(int(nd[i]), np.zeros(2 * int(nd[i])), p[i])
        A = np.asarray(flat, dtype=np.float64).reshape(4, 4)
        jtj[i] = [A[r, c] for r, c in UPPER]
        sig[i] = np.sqrt(np.diag(np.linalg.inv(A)))
    assert np.isfinite(sig).all() and np.isfinite(out["mprec_80"]).all() and np.isfinite(out["crlb"]).all()
    out["rnd_p"], out["rnd_nd"], out["rnd_jtj"], out["rnd_sig"] = p, nd, jtj, sig
    path = os.path.join(HERE, "fisher.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
