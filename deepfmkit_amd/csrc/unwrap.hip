// unwrap.hip — dfmi_unwrap's kernels and their launch (unwrap.h; include/dfmi.h).
//
// A tile is kUwTile = 1,024 points of one series: lane l of a 256-thread workgroup holds the
// kUwPer = 4 consecutive points 4 l .. 4 l + 3 (two 16-B loads where the rows are 16-B aligned,
// VEC; four single loads otherwise). A lane first folds its own points into a state and keeps
// the count of every point relative to its first valid one in registers (rel), so no jump is
// formed twice. The 64 lane states are scanned inside the wave by lane shuffles (six steps, no
// LDS memory), the four wave states cross through 4 x 32 B of LDS and one barrier, and the
// exclusive prefix of a lane is carry (everything before the tile) + waves before + lanes before.
//
//   unwrap_series_kernel   one workgroup per series walks the tiles in order, the carry in
//                          registers; the next tile's loads are issued before the current tile
//                          is scanned. Samples are read once, y and cycles written once.
//   unwrap_tile_kernel     tiled path, launch 1: the state of every tile (grid nser x ntile)
//   unwrap_carry_kernel    launch 2: one workgroup per series turns its tile states into
//                          exclusive carries in place, 256 tiles per step, and notes the series'
//                          first valid sample (the value a leading gap holds)
//   unwrap_apply_kernel    launch 3: a tile is re-read, scanned again and stored from its carry
//
// No workgroup waits for another: the three launches are the only synchronisation between
// workgroups, and the series kernel's workgroups share nothing.
#include <hip/hip_runtime.h>

#include "unwrap.h"

namespace dfmi {

namespace {

typedef double uw_d2 __attribute__((ext_vector_type(2)));
typedef long uw_l2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ UwState uw_shfl_up(const UwState& s, int d) {
  UwState r;
  r.sum = __shfl_up((long long)s.sum, d);
  r.first = __shfl_up(s.first, d);
  r.last = __shfl_up(s.last, d);
  r.has = __shfl_up(s.has, d);
  r.pad = 0;
  return r;
}

// The four points of one lane: samples (NaN past the end of the series: never valid) and validity.
struct UwPoints {
  double x[kUwPer];
  uint32_t ok;  // bit k: point k is valid
};

// A state that is the same in every lane of the wave, moved to scalar registers.
__device__ __forceinline__ UwState uw_uniform(const UwState& s) {
  const auto u32 = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
  const auto f64 = [&](double v) {
    return __hiloint2double((int)u32((uint32_t)__double2hiint(v)), (int)u32((uint32_t)__double2loint(v)));
  };
  UwState r;
  r.sum = (int64_t)(((uint64_t)u32((uint32_t)((uint64_t)s.sum >> 32)) << 32) | u32((uint32_t)s.sum));
  r.first = f64(s.first);
  r.last = f64(s.last);
  r.has = (int32_t)u32((uint32_t)s.has);
  r.pad = 0;
  return r;
}

// Rows are addressed from the tile's first point (a pointer that is the same in every lane) by a
// lane's 32-bit offset i0 = 4 tid; N counts the points from there to the end of the series.
template <bool VEC>
__device__ __forceinline__ void uw_load(const double* __restrict__ xr, const int32_t* __restrict__ sr, uint32_t i0,
                                        uint32_t N, int32_t max_status, UwPoints& p) {
  int32_t s[kUwPer];
  p.ok = 0;
  if (VEC && i0 + kUwPer <= N) {
    const uw_d2 a = *reinterpret_cast<const uw_d2*>(xr + i0), b = *reinterpret_cast<const uw_d2*>(xr + i0 + 2);
    p.x[0] = a[0], p.x[1] = a[1], p.x[2] = b[0], p.x[3] = b[1];
#pragma unroll
    for (int k = 0; k < kUwPer; ++k) s[k] = sr ? sr[i0 + k] : 0;
  } else {
#pragma unroll
    for (int k = 0; k < kUwPer; ++k) {
      const bool in = i0 + k < N;
      p.x[k] = in ? xr[i0 + k] : __builtin_nan("");
      s[k] = in && sr ? sr[i0 + k] : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < kUwPer; ++k) p.ok |= uw_valid(p.x[k], sr != nullptr, s[k], max_status) ? 1u << k : 0u;
}

// The state of a lane's own points; rel[k]: the count of point k relative to the lane's first
// valid point (held over invalid points).
__device__ __forceinline__ UwState uw_local(const UwPoints& p, double P, int64_t (&rel)[kUwPer]) {
  UwState loc = uw_identity();
#pragma unroll
  for (int k = 0; k < kUwPer; ++k) {
    if (p.ok >> k & 1) {
      if (loc.has) loc.sum += uw_jump(loc.last, p.x[k], P);
      else loc.first = p.x[k];
      loc.last = p.x[k];
      loc.has = 1;
    }
    rel[k] = loc.sum;
  }
  return loc;
}

// Scan of the workgroup's 256 states in thread order: excl = the threads before this one,
// total = all of them. lds: 4 states, free again after the caller's next barrier on another buffer.
__device__ __forceinline__ void uw_block_scan(UwState inc, double P, UwState* lds, UwState& excl, UwState& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const UwState l = uw_shfl_up(inc, d);
    if (lane >= d) inc = uw_combine(l, inc, P);
  }
  UwState ex = uw_shfl_up(inc, 1);
  if (lane == 0) ex = uw_identity();
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  UwState before = uw_identity();
  total = uw_identity();
#pragma unroll
  for (int w = 0; w < kUwThreads / 64; ++w) {
    const UwState s = uw_uniform(lds[w]);
    if (w < wave) before = uw_combine(before, s, P);
    total = uw_combine(total, s, P);
  }
  total = uw_uniform(total);
  excl = uw_combine(uw_uniform(before), ex, P);
}

// Stores a lane's four points. pre: the state of everything before the lane in its series;
// lead: the series' first valid sample (NaN when it has none), what a leading gap holds.
template <bool VEC>
__device__ __forceinline__ void uw_emit(const UwPoints& p, const UwState& loc, const int64_t (&rel)[kUwPer],
                                        const UwState& pre, double lead, double P, int32_t fill, uint32_t i0,
                                        uint32_t N, double* __restrict__ yr, int64_t* __restrict__ cr) {
  int64_t base = 0, hc = 0;
  double hy = fma(0.0, P, lead);
  if (pre.has) {
    base = loc.has ? pre.sum + uw_jump(pre.last, loc.first, P) : pre.sum;
    hc = pre.sum;
    hy = fma((double)pre.sum, P, pre.last);
  }
  double yv[kUwPer];
  int64_t cv[kUwPer];
#pragma unroll
  for (int k = 0; k < kUwPer; ++k) {
    const bool ok = p.ok >> k & 1;
    if (ok) {
      hc = base + rel[k];
      hy = fma((double)hc, P, p.x[k]);
    }
    cv[k] = hc;
    yv[k] = ok || fill ? hy : __builtin_nan("");
  }
  if (VEC && i0 + kUwPer <= N) {
    if (yr) {
      __builtin_nontemporal_store(uw_d2{yv[0], yv[1]}, reinterpret_cast<uw_d2*>(yr + i0));
      __builtin_nontemporal_store(uw_d2{yv[2], yv[3]}, reinterpret_cast<uw_d2*>(yr + i0 + 2));
    }
    if (cr) {
      __builtin_nontemporal_store(uw_l2{cv[0], cv[1]}, reinterpret_cast<uw_l2*>(cr + i0));
      __builtin_nontemporal_store(uw_l2{cv[2], cv[3]}, reinterpret_cast<uw_l2*>(cr + i0 + 2));
    }
  } else {
#pragma unroll
    for (int k = 0; k < kUwPer; ++k) {
      if (i0 + k < N) {
        if (yr) yr[i0 + k] = yv[k];
        if (cr) cr[i0 + k] = cv[k];
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kUwThreads) void unwrap_series_kernel(
    const double* __restrict__ x, int64_t ser_stride, int64_t N, double P, const int32_t* __restrict__ status,
    int64_t status_stride, int32_t max_status, int32_t fill, double* __restrict__ y, int64_t y_stride,
    int64_t* __restrict__ cycles, int64_t cycles_stride) {
  __shared__ UwState lds[2][kUwThreads / 64];
  __shared__ int32_t first_at[2][kUwThreads / 64];
  const int64_t r = blockIdx.x;
  const double* xr = x + r * ser_stride;
  const int32_t* sr = status ? status + r * status_stride : nullptr;
  double* yr = y ? y + r * y_stride : nullptr;
  int64_t* cr = cycles ? cycles + r * cycles_stride : nullptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t o = tid * kUwPer;
  const int64_t ntile = unwrap_ntile(N);
  UwPoints cur, nxt;

  // the value a leading gap holds: the first valid sample, found tile by tile (tile 0 when
  // point 0 is valid, so the search re-reads one tile)
  double lead = __builtin_nan("");
  if (fill && yr) {
    for (int64_t t = 0; t < ntile; ++t) {
      const int64_t b = t * kUwTile;
      uw_load<VEC>(xr + b, sr ? sr + b : nullptr, o, (uint32_t)(N - b), max_status, cur);
      int32_t at = 0x7fffffff;
#pragma unroll
      for (int k = kUwPer - 1; k >= 0; --k)
        if (cur.ok >> k & 1) at = (int32_t)(b + o + k);
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) at = min(at, __shfl_xor(at, o));
      if (lane == 0) first_at[t & 1][wave] = at;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < kUwThreads / 64; ++w) at = min(at, first_at[t & 1][w]);
      if (at != 0x7fffffff) {  // the same for every thread
        lead = xr[__builtin_amdgcn_readfirstlane(at)];
        break;
      }
    }
  }

  UwState carry = uw_identity();
  uw_load<VEC>(xr, sr, o, (uint32_t)N, max_status, cur);
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t b = t * kUwTile, bn = b + kUwTile;
    if (t + 1 < ntile) uw_load<VEC>(xr + bn, sr ? sr + bn : nullptr, o, (uint32_t)(N - bn), max_status, nxt);
    int64_t rel[kUwPer];
    const UwState loc = uw_local(cur, P, rel);
    UwState excl, total;
    uw_block_scan(loc, P, lds[t & 1], excl, total);
    uw_emit<VEC>(cur, loc, rel, uw_combine(carry, excl, P), lead, P, fill, o, (uint32_t)(N - b), yr ? yr + b : nullptr,
                 cr ? cr + b : nullptr);
    carry = uw_uniform(uw_combine(carry, total, P));
    cur = nxt;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kUwThreads, 8) void unwrap_tile_kernel(const double* __restrict__ x, int64_t ser_stride,
                                                                 int64_t N, double P,
                                                                 const int32_t* __restrict__ status,
                                                                 int64_t status_stride, int32_t max_status,
                                                                 int32_t ntile, UwState* __restrict__ tiles) {
  __shared__ UwState lds[kUwThreads / 64];
  const int64_t r = blockIdx.x / ntile, b = (int64_t)(blockIdx.x % ntile) * kUwTile;
  UwPoints pts;
  uw_load<VEC>(x + r * ser_stride + b, status ? status + r * status_stride + b : nullptr, threadIdx.x * kUwPer,
               (uint32_t)(N - b), max_status, pts);
  int64_t rel[kUwPer];
  UwState excl, total;
  uw_block_scan(uw_local(pts, P, rel), P, lds, excl, total);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(kUwThreads, 8) void unwrap_carry_kernel(UwState* __restrict__ tiles, int32_t ntile, double P,
                                                                  double* __restrict__ lead) {
  __shared__ UwState lds[2][kUwThreads / 64];
  UwState* row = tiles + (int64_t)blockIdx.x * ntile;
  const int tid = threadIdx.x;
  UwState carry = uw_identity();
  UwState cur = tid < ntile ? row[tid] : uw_identity();
  for (int32_t b = 0, step = 0; b < ntile; b += kUwThreads, ++step) {
    const int32_t n = b + kUwThreads + tid;
    const UwState nxt = n < ntile ? row[n] : uw_identity();
    UwState excl, total;
    uw_block_scan(cur, P, lds[step & 1], excl, total);
    if (b + tid < ntile) row[b + tid] = uw_combine(carry, excl, P);
    carry = uw_uniform(uw_combine(carry, total, P));
    cur = nxt;
  }
  if (tid == 0) lead[blockIdx.x] = carry.has ? carry.first : __builtin_nan("");
}

template <bool VEC>
__global__ __launch_bounds__(kUwThreads, 8) void unwrap_apply_kernel(
    const double* __restrict__ x, int64_t ser_stride, int64_t N, double P, const int32_t* __restrict__ status,
    int64_t status_stride, int32_t max_status, int32_t fill, double* __restrict__ y, int64_t y_stride,
    int64_t* __restrict__ cycles, int64_t cycles_stride, int32_t ntile, const UwState* __restrict__ tiles,
    const double* __restrict__ lead) {
  __shared__ UwState lds[kUwThreads / 64];
  const int64_t r = blockIdx.x / ntile, b = (int64_t)(blockIdx.x % ntile) * kUwTile;
  const uint32_t o = threadIdx.x * kUwPer, n = (uint32_t)(N - b);
  UwPoints pts;
  uw_load<VEC>(x + r * ser_stride + b, status ? status + r * status_stride + b : nullptr, o, n, max_status, pts);
  int64_t rel[kUwPer];
  const UwState loc = uw_local(pts, P, rel);
  UwState excl, total;
  uw_block_scan(loc, P, lds, excl, total);
  const UwState* c = tiles + blockIdx.x;
  const UwState carry = {c->sum, c->first, c->last, c->has, 0};
  uw_emit<VEC>(pts, loc, rel, uw_combine(carry, excl, P), lead[r], P, fill, o, n,
               y ? y + r * y_stride + b : nullptr, cycles ? cycles + r * cycles_stride + b : nullptr);
}

template <bool VEC>
hipError_t unwrap_launch_t(const double* x, int64_t nser, int64_t ser_stride, int64_t N, double P,
                           const int32_t* status, int64_t status_stride, int32_t max_status, int32_t fill, double* y,
                           int64_t y_stride, int64_t* cycles, int64_t cycles_stride, int path, UwState* tiles,
                           double* lead, hipStream_t st) {
  const dim3 wg(kUwThreads);
  if (path == 1) {
    hipLaunchKernelGGL(unwrap_series_kernel<VEC>, dim3((unsigned)nser), wg, 0, st, x, ser_stride, N, P, status,
                       status_stride, max_status, fill, y, y_stride, cycles, cycles_stride);
    return hipGetLastError();
  }
  const int32_t ntile = (int32_t)unwrap_ntile(N);
  const dim3 grid((unsigned)(nser * ntile));
  hipLaunchKernelGGL(unwrap_tile_kernel<VEC>, grid, wg, 0, st, x, ser_stride, N, P, status, status_stride, max_status,
                     ntile, tiles);
  hipLaunchKernelGGL(unwrap_carry_kernel, dim3((unsigned)nser), wg, 0, st, tiles, ntile, P, lead);
  hipLaunchKernelGGL(unwrap_apply_kernel<VEC>, grid, wg, 0, st, x, ser_stride, N, P, status, status_stride, max_status,
                     fill, y, y_stride, cycles, cycles_stride, ntile, (const UwState*)tiles, (const double*)lead);
  return hipGetLastError();
}

}  // namespace

hipError_t unwrap_launch(const double* x, int64_t nser, int64_t ser_stride, int64_t N, double P,
                         const int32_t* status, int64_t status_stride, int32_t max_status, int32_t fill, double* y,
                         int64_t y_stride, int64_t* cycles, int64_t cycles_stride, int path, UwState* tiles,
                         double* lead, hipStream_t st) {
  if (nser <= 0 || N <= 0) return hipSuccess;
  // 16-B loads and stores where every row of x, y and cycles starts on a 16-B boundary
  const bool many = nser > 1;
  const bool vec = ((uintptr_t)x & 15) == 0 && (!many || ser_stride % 2 == 0) &&
                   (!y || (((uintptr_t)y & 15) == 0 && (!many || y_stride % 2 == 0))) &&
                   (!cycles || (((uintptr_t)cycles & 15) == 0 && (!many || cycles_stride % 2 == 0)));
  if (vec)
    return unwrap_launch_t<true>(x, nser, ser_stride, N, P, status, status_stride, max_status, fill, y, y_stride, cycles,
                                 cycles_stride, path, tiles, lead, st);
  return unwrap_launch_t<false>(x, nser, ser_stride, N, P, status, status_stride, max_status, fill, y, y_stride, cycles,
                                cycles_stride, path, tiles, lead, st);
}

}  // namespace dfmi
