// hostcheck_fisher.hip — TEST-ONLY host build of deepfmkit_amd/csrc/fisher.h: the point
// function dfmi_fisher's kernel runs per lane (fisher_point is __host__ __device__), over
// arrays, in dfmi_fisher's layouts, so the CPU suite can gate J^T J, the covariance, the
// standard errors and the singularity rule without a GPU. The product library never links
// this; tests/test_gpu_fisher.py exercises the real kernel.
#include "../../deepfmkit_amd/csrc/fisher.h"

extern "C" {

// params[i*ld + s]; var NULL or [s]; jtj / cov [k*n + s], sigma [i*n + s], ok [s]; NULL = skipped
void hc_fisher(const double* params, int64_t n, int64_t ld, int32_t ndata, const double* var, double var_mul,
               double* jtj, double* cov, double* sigma, int32_t* ok) {
  for (int64_t s = 0; s < n; ++s) {
    dfmi::FisherPoint o;
    dfmi::fisher_point(params[s], params[ld + s], params[2 * ld + s], params[3 * ld + s], ndata,
                       var ? var[s] * var_mul : var_mul, o);
    const double a[10] = {o.a00, o.a01, o.a02, o.a03, o.a11, o.a12, o.a13, o.a22, o.a23, o.a33};
    const double c[10] = {o.c00, o.c01, o.c02, o.c03, o.c11, o.c12, o.c13, o.c22, o.c23, o.c33};
    const double sg[4] = {o.s0, o.s1, o.s2, o.s3};
    for (int k = 0; k < 10; ++k) {
      if (jtj) jtj[k * n + s] = a[k];
      if (cov) cov[k * n + s] = c[k];
    }
    for (int i = 0; i < 4; ++i)
      if (sigma) sigma[i * n + s] = sg[i];
    if (ok) ok[s] = o.ok;
  }
}

}  // extern "C"
