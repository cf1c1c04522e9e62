// residual.hip — residual_kernel's instantiations and launch (residual.h; include/dfmi.h
// dfmi_residual). Sample type x {16-B loads, single-sample loads} x {periodic, rotating}.
#include <hip/hip_runtime.h>

#include "../../include/dfmi.h"
#include "residual.h"

namespace dfmi {

namespace {

template <typename XT, int VEC, bool PERIODIC>
hipError_t residual_launch_t(const XT* x, int64_t nseg, int64_t seg_stride, int R, double w0, int L,
                             const double* params, int64_t ld, const double* dc, double* rss, double* peak,
                             int32_t* ipeak, double* resid, int64_t resid_stride, int n_cu, hipStream_t st) {
  auto kern = residual_kernel<XT, VEC, PERIODIC>;
  const size_t lds = PERIODIC ? (size_t)kResWaves * L * sizeof(double) : 0;
  int per_cu = 0;
  if (hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 64 * kResWaves, lds); e != hipSuccess)
    return e;
  if (per_cu < 1) per_cu = 1;
  const int64_t need = (nseg + kResWaves - 1) / kResWaves;
  int64_t grid = (int64_t)n_cu * per_cu;
  if (grid > need) grid = need;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * kResWaves), lds, st, x, nseg, seg_stride, R, w0, L, params, ld,
                     dc, rss, peak, ipeak, resid, resid_stride);
  return hipGetLastError();
}

// 16-B loads and stores where every sample row and every residual row starts on a 16-B
// boundary; else one sample per lane and load.
template <typename XT>
hipError_t residual_launch_x(const XT* x, int64_t nseg, int64_t seg_stride, int R, double w0, int L,
                             const double* params, int64_t ld, const double* dc, double* rss, double* peak,
                             int32_t* ipeak, double* resid, int64_t resid_stride, int n_cu, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(XT);
  const bool vec = ((uintptr_t)x & 15) == 0 && (nseg == 1 || seg_stride % V == 0) &&
                   (!resid || (((uintptr_t)resid & 15) == 0 && (nseg == 1 || resid_stride % 2 == 0)));
#define DFMI_RESIDUAL(V_, P_)                                                                                      \
  return residual_launch_t<XT, V_, P_>(x, nseg, seg_stride, R, w0, L, params, ld, dc, rss, peak, ipeak, resid, \
                                       resid_stride, n_cu, st)
  if (L > 0) {
    if (vec) DFMI_RESIDUAL(V, true);
    DFMI_RESIDUAL(1, true);
  }
  if (vec) DFMI_RESIDUAL(V, false);
  DFMI_RESIDUAL(1, false);
#undef DFMI_RESIDUAL
}

}  // namespace

hipError_t residual_launch(const void* x, int xtype, int64_t nseg, int64_t seg_stride, int R, double w0, int L,
                           const double* params, int64_t ld, const double* dc, double* rss, double* peak,
                           int32_t* ipeak, double* resid, int64_t resid_stride, int n_cu, hipStream_t st) {
  if (nseg <= 0) return hipSuccess;
  if (xtype == DFMI_F32)
    return residual_launch_x((const float*)x, nseg, seg_stride, R, w0, L, params, ld, dc, rss, peak, ipeak, resid,
                             resid_stride, n_cu, st);
  if (xtype == DFMI_I16)
    return residual_launch_x((const int16_t*)x, nseg, seg_stride, R, w0, L, params, ld, dc, rss, peak, ipeak, resid,
                             resid_stride, n_cu, st);
  return residual_launch_x((const double*)x, nseg, seg_stride, R, w0, L, params, ld, dc, rss, peak, ipeak, resid,
                           resid_stride, n_cu, st);
}

}  // namespace dfmi
