// fisher.hip — dfmi_fisher's kernel: J^T J, covariance and standard errors of the DFMI model
// at n parameter points (fisher.h), one lane per point.
//   params[i*ld + s], i < 4   amp, m, phi, psi of point s (dfmi_lm's / dfmi_nls_record's layout)
//   var[s] (or NULL) * var_mul  the variance factor of point s
//   jtj[k*n + s], cov[k*n + s], k < 10 (00 01 02 03 11 12 13 22 23 33), sigma[i*n + s], ok[s]
// Every output is component-major, so a wave stores each component coalesced; NULL outputs
// are skipped (a uniform branch: the pointers are kernel arguments).
#include <hip/hip_runtime.h>

#include "fisher.h"

namespace dfmi {

__global__ __launch_bounds__(64) void fisher_kernel(const double* __restrict__ params, int64_t n, int64_t ld,
                                                    int ndata, const double* __restrict__ var, double var_mul,
                                                    double* __restrict__ jtj, double* __restrict__ cov,
                                                    double* __restrict__ sigma, int32_t* __restrict__ ok) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const double a = params[s], m = params[ld + s], phi = params[2 * ld + s], psi = params[3 * ld + s];
  const double v = var ? var[s] * var_mul : var_mul;
  FisherPoint o;
  fisher_point(a, m, phi, psi, ndata, v, o);
  if (jtj) {
    jtj[s] = o.a00;
    jtj[n + s] = o.a01;
    jtj[2 * n + s] = o.a02;
    jtj[3 * n + s] = o.a03;
    jtj[4 * n + s] = o.a11;
    jtj[5 * n + s] = o.a12;
    jtj[6 * n + s] = o.a13;
    jtj[7 * n + s] = o.a22;
    jtj[8 * n + s] = o.a23;
    jtj[9 * n + s] = o.a33;
  }
  if (cov) {
    cov[s] = o.c00;
    cov[n + s] = o.c01;
    cov[2 * n + s] = o.c02;
    cov[3 * n + s] = o.c03;
    cov[4 * n + s] = o.c11;
    cov[5 * n + s] = o.c12;
    cov[6 * n + s] = o.c13;
    cov[7 * n + s] = o.c22;
    cov[8 * n + s] = o.c23;
    cov[9 * n + s] = o.c33;
  }
  if (sigma) {
    sigma[s] = o.s0;
    sigma[n + s] = o.s1;
    sigma[2 * n + s] = o.s2;
    sigma[3 * n + s] = o.s3;
  }
  if (ok) ok[s] = o.ok;
}

hipError_t fisher_launch(const double* params, int64_t n, int64_t ld, int ndata, const double* var, double var_mul,
                         double* jtj, double* cov, double* sigma, int32_t* ok, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(fisher_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, params, n, ld, ndata, var,
                     var_mul, jtj, cov, sigma, ok);
  return hipGetLastError();
}

}  // namespace dfmi
