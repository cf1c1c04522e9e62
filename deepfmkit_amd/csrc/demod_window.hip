// demod_window.hip — the instances of demod_window_kernel (demod_window.h) and their launch, in a
// translation unit of their own: 36 instances (VEC 1 / 2, MAXSLOT 2 / 4, K 1 / 2 / 3, three sample
// types) compile beside dfmi_capi.hip instead of lengthening it, and the debug and A/B builds of
// dfmi_capi.hip link this object as it is. The host side (tables, geometry, grid) stays in dfmi_capi.hip.
// demod.h defines one kernel that is no template, demod_direct_kernel, which dfmi_capi.hip launches: this
// unit's (unused) copy of it takes another name, or the two objects would not link.
#define demod_direct_kernel demod_direct_kernel_in_window_unit
#include "demod_window.h"
#undef demod_direct_kernel

#include "../../include/dfmi.h"

namespace dfmi {

namespace {

// f(kernel) for the instance (VEC, MAXSLOT, K) of sample type XT; hipErrorInvalidValue for any other triple.
template <typename XT, typename F>
hipError_t with_window_kernel(int vec, int ms, int K, F f) {
#define DFMI_WIN(V_, M_, K_) \
  if (vec == V_ && ms == M_ && K == K_) return f(demod_window_kernel<V_, M_, K_, XT>)
#define DFMI_WIN_K(V_, M_) \
  DFMI_WIN(V_, M_, 1);     \
  DFMI_WIN(V_, M_, 2);     \
  DFMI_WIN(V_, M_, 3)
  DFMI_WIN_K(1, 2);
  DFMI_WIN_K(1, 4);
  DFMI_WIN_K(2, 2);
  DFMI_WIN_K(2, 4);
#undef DFMI_WIN_K
#undef DFMI_WIN
  return hipErrorInvalidValue;
}

template <typename F>
hipError_t with_window_type(int xtype, int vec, int ms, int K, F f) {
  if (xtype == DFMI_F64) return with_window_kernel<double>(vec, ms, K, [&](auto k) { return f(k, (const double*)nullptr); });
  if (xtype == DFMI_F32) return with_window_kernel<float>(vec, ms, K, [&](auto k) { return f(k, (const float*)nullptr); });
  if (xtype == DFMI_I16) return with_window_kernel<int16_t>(vec, ms, K, [&](auto k) { return f(k, (const int16_t*)nullptr); });
  return hipErrorInvalidValue;
}

}  // namespace

// Resident workgroups per CU of the instance at `lds` bytes of dynamic LDS.
hipError_t window_occupancy(int xtype, int vec, int ms, int K, size_t lds, int* per_cu) {
  return with_window_type(xtype, vec, ms, K, [&](auto kern, auto) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, kern, kBlockThreads, lds);
  });
}

// Launch of the instance on `grid` workgroups; x points to samples of type xtype.
hipError_t window_launch(int xtype, int vec, int ms, int K, int64_t grid, size_t lds, hipStream_t st, const void* x,
                         int64_t nseg, int64_t seg_stride, int R, int L, int ndata, const double* tab,
                         const double* wcyc, const double* wbin, double* qi, int64_t qi_ld, double* dc) {
  return with_window_type(xtype, vec, ms, K, [&](auto kern, auto typed) {
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlockThreads), lds, st, (decltype(typed))x, nseg, seg_stride, R,
                       L, ndata, tab, wcyc, wbin, qi, qi_ld, dc);
    return hipGetLastError();
  });
}

}  // namespace dfmi
