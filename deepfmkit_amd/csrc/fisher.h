// fisher.h — the Fisher matrix J^T J of the DFMI model at one parameter point and its
// inverse: per-segment parameter covariances / standard errors and the CRLB helpers
// (helpers.py:16-45, 98-132 of the reference; J^T J is coeffs', fit.py:68-150).
//
// The model Jacobian depends on (a, m, phi, psi) alone, never on the data, so one point
// function serves a fit (cov = ssq/(2 ndata - 4) (J^T J)^-1 at the fitted parameters) and
// the CRLB (cov = sigma_QI^2 (J^T J)^-1 at a chosen point).
//
//  * J^T J: the general path's pieces of lm.h: harmonic_walk (the two-pass Miller walk, the
//    series and the large-argument branches, cos/sin(j psi) by rotation) and harmonic_term
//    with Q = I = 0 (its residual sums are dead code here), hence quarter_turn and the
//    a == 0 rule of column 0 (fit.py:126-128). The ten sums are eval_gen's, bit for bit.
//  * inverse: A is equilibrated by its diagonal, B = D^-1/2 A D^-1/2 (unit diagonal: the
//    columns differ by orders of magnitude, d/dpsi carries a factor j), B = L L^T by an
//    unrolled Cholesky, B^-1 = L^-T L^-1, cov = var D^-1/2 B^-1 D^-1/2, sigma_i = sqrt(cov_ii).
//    Everything is named scalars: no private array is indexed at run time.
//  * a point is NOT OK when a parameter, var or a diagonal entry is non-finite, var is
//    negative (no covariance: sigma would be the root of a negative number), a diagonal
//    entry is <= 0 or a Cholesky pivot is <= 0 (a = 0, m = 0: the reference's LinAlgError):
//    cov and sigma are NaN, ok = 0, J^T J is still what was computed. So sigma and cov are
//    NaN exactly where ok = 0.
#pragma once
#include "dfmi_math.h"
#include "lm.h"

namespace dfmi {

struct FisherPoint {
  double a00, a01, a02, a03, a11, a12, a13, a22, a23, a33;  // J^T J (upper)
  double c00, c01, c02, c03, c11, c12, c13, c22, c23, c33;  // covariance (upper)
  double s0, s1, s2, s3;                                    // standard errors
  int ok;
};

DFMI_HDI bool fisher_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN, +-inf

// J^T J of fit.py:68-150 at (a, m, phi, psi) for ndata harmonics (eval_gen's sums).
DFMI_HDI void fisher_jtj(double a, double m, double phi, double psi, int ndata, Eval& e) {
  double sph, cph;
  sincos(phi, &sph, &cph);
  const bool a_nz = (a != 0.0);
  eval_zero(e);
  harmonic_walk(ndata, m, psi, [&](int j, double Jm1, double J0, double Jp1, double cj, double sj) {
    harmonic_term(e, j, a, a_nz, cph, sph, Jm1, J0, Jp1, cj, sj, 0.0, 0.0);
  });
}

DFMI_HDI void fisher_point(double a, double m, double phi, double psi, int ndata, double var, FisherPoint& o) {
  Eval e;
  fisher_jtj(a, m, phi, psi, ndata, e);
  o.a00 = e.a00; o.a01 = e.a01; o.a02 = e.a02; o.a03 = e.a03; o.a11 = e.a11;
  o.a12 = e.a12; o.a13 = e.a13; o.a22 = e.a22; o.a23 = e.a23; o.a33 = e.a33;
  bool ok = fisher_finite(a) && fisher_finite(m) && fisher_finite(phi) && fisher_finite(psi) && fisher_finite(var);
  ok = ok && var >= 0.0;
  ok = ok && fisher_finite(e.a00) && fisher_finite(e.a11) && fisher_finite(e.a22) && fisher_finite(e.a33);
  ok = ok && e.a00 > 0.0 && e.a11 > 0.0 && e.a22 > 0.0 && e.a33 > 0.0;
  // D^-1/2 (1 where the point is already lost: nothing below may trap or divide by 0)
  const double d0 = ok ? 1.0 / sqrt(e.a00) : 1.0, d1 = ok ? 1.0 / sqrt(e.a11) : 1.0;
  const double d2 = ok ? 1.0 / sqrt(e.a22) : 1.0, d3 = ok ? 1.0 / sqrt(e.a33) : 1.0;
  // B = D^-1/2 A D^-1/2, unit diagonal; lower triangle b10 .. b32
  const double b10 = e.a01 * d0 * d1, b20 = e.a02 * d0 * d2, b30 = e.a03 * d0 * d3;
  const double b21 = e.a12 * d1 * d2, b31 = e.a13 * d1 * d3, b32 = e.a23 * d2 * d3;
  // Cholesky B = L L^T (l00 = 1)
  const double p1 = fma(-b10, b10, 1.0);
  ok = ok && p1 > 0.0;
  const double l11 = sqrt(ok ? p1 : 1.0), r11 = 1.0 / l11;
  const double l21 = fma(-b20, b10, b21) * r11;
  const double l31 = fma(-b30, b10, b31) * r11;
  const double p2 = fma(-l21, l21, fma(-b20, b20, 1.0));
  ok = ok && p2 > 0.0;
  const double l22 = sqrt(ok ? p2 : 1.0), r22 = 1.0 / l22;
  const double l32 = fma(-l31, l21, fma(-b30, b20, b32)) * r22;
  const double p3 = fma(-l32, l32, fma(-l31, l31, fma(-b30, b30, 1.0)));
  ok = ok && p3 > 0.0;
  const double l33 = sqrt(ok ? p3 : 1.0), r33 = 1.0 / l33;
  // M = L^-1 (lower, m00 = 1)
  const double m11 = r11, m22 = r22, m33 = r33;
  const double m10 = -b10 * r11;
  const double m21 = -l21 * m11 * r22;
  const double m20 = -fma(l21, m10, b20) * r22;
  const double m32 = -l32 * m22 * r33;
  const double m31 = -fma(l32, m21, l31 * m11) * r33;
  const double m30 = -fma(l32, m20, fma(l31, m10, b30)) * r33;
  // B^-1 = M^T M
  const double x00 = fma(m30, m30, fma(m20, m20, fma(m10, m10, 1.0)));
  const double x01 = fma(m30, m31, fma(m20, m21, m10 * m11));
  const double x02 = fma(m30, m32, m20 * m22);
  const double x03 = m30 * m33;
  const double x11 = fma(m31, m31, fma(m21, m21, m11 * m11));
  const double x12 = fma(m31, m32, m21 * m22);
  const double x13 = m31 * m33;
  const double x22 = fma(m32, m32, m22 * m22);
  const double x23 = m32 * m33;
  const double x33 = m33 * m33;
  const double nan = __builtin_nan("");
  const double v0 = var * d0, v1 = var * d1, v2 = var * d2, v3 = var * d3;
  o.c00 = ok ? x00 * v0 * d0 : nan;
  o.c01 = ok ? x01 * v0 * d1 : nan;
  o.c02 = ok ? x02 * v0 * d2 : nan;
  o.c03 = ok ? x03 * v0 * d3 : nan;
  o.c11 = ok ? x11 * v1 * d1 : nan;
  o.c12 = ok ? x12 * v1 * d2 : nan;
  o.c13 = ok ? x13 * v1 * d3 : nan;
  o.c22 = ok ? x22 * v2 * d2 : nan;
  o.c23 = ok ? x23 * v2 * d3 : nan;
  o.c33 = ok ? x33 * v3 * d3 : nan;
  o.s0 = ok ? sqrt(o.c00) : nan;
  o.s1 = ok ? sqrt(o.c11) : nan;
  o.s2 = ok ? sqrt(o.c22) : nan;
  o.s3 = ok ? sqrt(o.c33) : nan;
  o.ok = ok ? 1 : 0;
}

// Launch of fisher_kernel (fisher.hip): one lane per point, see include/dfmi.h dfmi_fisher.
hipError_t fisher_launch(const double* params, int64_t n, int64_t ld, int ndata, const double* var, double var_mul,
                         double* jtj, double* cov, double* sigma, int32_t* ok, hipStream_t st);

}  // namespace dfmi
