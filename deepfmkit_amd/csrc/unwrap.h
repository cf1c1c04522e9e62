// unwrap.h — phase unwrapping of series with gaps as an exact integer scan (dfmi_unwrap;
// DESIGN.md §21). The point functions: the jump rule, the state of a run of points and its
// combine, __host__ __device__ so that host and device share one text; unwrap.hip holds the
// kernels.
//
//   valid points v0 < v1 < ... of a series, P = period:
//   c[v0] = 0,  c[v_j] = c[v_{j-1}] - rint((x[v_j] - x[v_{j-1}]) / P)   (double, half to even)
//   y[v] = fma((double)c[v], P, x[v])
//
// The state of a run of consecutive points is {sum of the jumps inside the run, its first and
// its last valid sample, whether it has one}. Two adjacent runs combine to sum_a + sum_b +
// jump(last_a, first_b): associative, and exact because the sums are integers, so any split of
// a series into lanes, waves, tiles and launches gives the same counts.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef DFMI_HDI
#define DFMI_HDI __host__ __device__ __forceinline__
#endif

namespace dfmi {

constexpr int kUwThreads = 256;                // one workgroup: 4 waves
constexpr int kUwPer = 4;                      // consecutive points per lane
constexpr int kUwTile = kUwThreads * kUwPer;   // points per tile (1,024)

struct UwState {
  int64_t sum;         // sum of the jumps between the run's valid points
  double first, last;  // its first and last valid sample (unspecified when has == 0)
  int32_t has;         // 1 when the run holds a valid point
  int32_t pad;
};

DFMI_HDI UwState uw_identity() { return UwState{0, 0.0, 0.0, 0, 0}; }

// Cycles the count changes by from a valid sample to the next valid one.
DFMI_HDI int64_t uw_jump(double prev, double cur, double P) {
  const double d = cur - prev;
  return -(int64_t)rint(d / P);
}

DFMI_HDI bool uw_valid(double x, bool with_status, int32_t s, int32_t max_status) {
  return fabs(x) <= 1.7976931348623157e308 && (!with_status || (s >= 0 && s <= max_status));
}

// The state of run a followed by run b.
DFMI_HDI UwState uw_combine(const UwState& a, const UwState& b, double P) {
  if (!a.has) return b;
  if (!b.has) return a;
  return UwState{a.sum + b.sum + uw_jump(a.last, b.first, P), a.first, b.last, 1, 0};
}

DFMI_HDI int64_t unwrap_ntile(int64_t N) { return (N + kUwTile - 1) / kUwTile; }

#if defined(__HIPCC__)
// Launches on st (unwrap.hip); device pointers, nser >= 1, 1 <= N < 2^31; y or cycles may be NULL.
//   path 1, the series kernel: one workgroup per series walks its tiles in order.
//   path 2, tiled: tile states (grid nser x ntile), one workgroup per series scans them into
//   exclusive carries and the series' first valid sample (lead), then the tiles are re-read and
//   stored. tiles: nser * unwrap_ntile(N) states, lead: nser doubles (path 2 only);
//   nser * unwrap_ntile(N) < 2^31.
hipError_t unwrap_launch(const double* x, int64_t nser, int64_t ser_stride, int64_t N, double P,
                         const int32_t* status, int64_t status_stride, int32_t max_status, int32_t fill, double* y,
                         int64_t y_stride, int64_t* cycles, int64_t cycles_stride, int path, UwState* tiles,
                         double* lead, hipStream_t st);
#endif

}  // namespace dfmi
