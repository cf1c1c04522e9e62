// residual.h — time-domain residual of the fitted DFMI model per segment (dfmi_residual).
//
// For a segment x[t], t < R, with fit results (a, m, phi, psi) and dc = mean(x):
//     theta_t = w0 t + psi,  ac(t) = a cos(phi + m cos(theta_t)),
//     k = dc - (1/R) sum_t ac(t),  r(t) = x(t) - k - ac(t)
// and the outputs are rss = sum r^2, peak = max |r|, ipeak = its t (the smallest on a tie) and,
// on request, r itself. The kernel is one pass over the samples: every sample is read once.
//
// Layout: one wavefront owns one segment at a time (persistent grid-stride), no exchange between
// waves. In iteration i lane l holds the VEC samples t = (64 i + l) VEC + e, e < VEC: one 16-B
// non-temporal load per lane where every row starts on a 16-B boundary (VEC = 16 / sizeof(XT):
// 2 doubles, 4 floats, 8 int16), else one sample per lane and load (VEC = 1: any base pointer, any
// seg_stride). UNR loads per lane are in flight before the first is used; float and int16
// samples are widened in registers. The residual, when wanted, leaves in 16-B stores (non-temporal
// where a lane's samples are one store, VEC = 2; cached where they are several, see the store).
//
// Two model evaluators stand behind the one sample loop:
//  * ResPeriodic (w0 L = 2 pi n, L <= kResMaxL): the wave builds A[p] = ac(p), p < L, in its own
//    LDS slice (L / 64 evaluations per lane) and forms k from it before any sample is touched,
//    k = dc - (1/R) sum_p cnt[p] A[p] with cnt[p] = #{t < R : t mod L = p} (zero for p >= R, so
//    R < L and a partial last cycle need no case of their own). In the loop a lane carries its
//    phase p forward by (64 VEC) mod L: one add and one compare, no division.
//  * ResRotating (no period): e^{i theta_t} is carried from sample to sample by one complex
//    multiplication (by e^{i w0} within a lane's VEC samples, by e^{i w0 64 VEC} between its
//    iterations) and re-anchored by an exact sincos at every group of UNR iterations, so a
//    value is at most UNR - 1 + VEC - 1 products away from an anchor. One cos(phi + m c) per
//    sample. The wave sums ac(t) in a pass without samples first (k), then makes the sample pass.
//
// rss does not depend on the sample type or on VEC: sample t adds r^2 into partial sum t mod 512
// of the wave (kResAcc = 8 per lane, whichever lane and register that is in a layout), each in
// ascending t, and the 512 are summed pairwise over the bits of t mod 512 from bit 0 up: a bit
// is a register pair or a lane swap by layout, and a + b = b + a exactly. So with ResPeriodic
// (whose ac(t) does not depend on the layout either) a float or int16 record gives the bits of the
// widened double record, aligned or not; ResRotating's products follow VEC. The peak's maximum is
// exact in any order; its reduction carries the index and keeps the smaller t on a tie.
//
// A non-finite a, m, phi, psi or dc: rss = peak = NaN, ipeak = -1, a NaN residual row. A
// non-finite sample propagates through r and rss; a NaN rss gives peak = NaN, ipeak = -1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace dfmi {

constexpr int kResWaves = 4;     // waves per workgroup
constexpr int kResAcc = 8;       // partial sums of r^2 per lane: 512 per wave, by t mod 512
constexpr int kResMaxL = 1024;   // largest period the LDS table holds (8 KB per wave)

__device__ __forceinline__ double res_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// LDS writes and reads of one wave's own table, ordered (no other wave touches it).
__device__ __forceinline__ void res_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

template <typename XT, int VEC>
struct ResRaw {
  typedef XT V __attribute__((ext_vector_type(VEC)));
  V v;
  __device__ __forceinline__ double at(int e) const { return (double)v[e]; }
};
template <typename XT>
struct ResRaw<XT, 1> {
  XT v;
  __device__ __forceinline__ double at(int) const { return (double)v; }
};

// The VEC samples from xs + t on (t a multiple of VEC, rows VEC-aligned when VEC > 1); zero past R.
template <typename XT, int VEC>
__device__ __forceinline__ void res_load(const XT* __restrict__ xs, int t, int R, ResRaw<XT, VEC>& raw) {
  if constexpr (VEC == 1) {
    raw.v = t < R ? __builtin_nontemporal_load(xs + t) : (XT)0;
  } else {
    using V = typename ResRaw<XT, VEC>::V;
    V r = (V)(XT)0;
    if (t + VEC <= R) {
      r = __builtin_nontemporal_load(reinterpret_cast<const V*>(xs + t));  // global_load_dwordx4 ... nt
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e)
        if (t + e < R) r[e] = xs[t + e];
    }
    raw.v = r;
  }
}

__device__ __forceinline__ double res_ac(double a, double m, double phi, double theta) {
  return a * cos(phi + m * cos(theta));
}

__device__ __forceinline__ bool res_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// ac(t) from the wave's LDS table; p = t mod L of the lane's next first sample.
struct ResPeriodic {
  const double* A;
  int L, p, dp;
  __device__ __forceinline__ void seek(int) {}
  template <int VEC>
  __device__ __forceinline__ void next(double (&ac)[VEC]) {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int q = p + e;  // e < VEC <= L
      ac[e] = A[q >= L ? q - L : q];
    }
    p += dp;
    p = p >= L ? p - L : p;
  }
};

// ac(t) with e^{i theta_t} carried by rotation from the anchor seek(t) set.
struct ResRotating {
  double a, m, phi, psi, w0;
  double c1, s1, cs, ss;  // e^{i w0}, e^{i w0 64 VEC}
  double c, s;            // e^{i theta} at the lane's next first sample
  __device__ __forceinline__ void seek(int t) { sincos(w0 * (double)t + psi, &s, &c); }
  template <int VEC>
  __device__ __forceinline__ void next(double (&ac)[VEC]) {
    double ce = c, se = s;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      ac[e] = a * cos(phi + m * ce);
      if (e + 1 < VEC) {
        const double cn = ce * c1 - se * s1;
        se = se * c1 + ce * s1;
        ce = cn;
      }
    }
    const double cn = c * cs - s * ss;
    s = s * cs + c * ss;
    c = cn;
  }
};

// The wave's 512 partial sums (register j = (iteration % ITS) VEC + e of lane l holds t mod 512 =
// (iteration % ITS) 64 VEC + l VEC + e) added pairwise over the bits of t mod 512, bit 0 first.
template <int VEC>
__device__ __forceinline__ double res_sum(double (&acc)[kResAcc]) {
#pragma unroll
  for (int b = 1; b < VEC; b <<= 1)
#pragma unroll
    for (int j = 0; j < kResAcc; j += 2 * b) acc[j] += acc[j + b];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
#pragma unroll
    for (int j = 0; j < kResAcc; j += VEC) acc[j] += __shfl_xor(acc[j], o);
#pragma unroll
  for (int b = VEC; b < kResAcc; b <<= 1)
#pragma unroll
    for (int j = 0; j < kResAcc; j += 2 * b) acc[j] += acc[j + b];
  return acc[0];
}

// Dynamic LDS: PERIODIC: kResWaves slices of L doubles.
template <typename XT, int VEC, bool PERIODIC>
__global__ __launch_bounds__(64 * kResWaves) void residual_kernel(
    const XT* __restrict__ x, int64_t nseg, int64_t seg_stride, int R, double w0, int L,
    const double* __restrict__ params, int64_t ld, const double* __restrict__ dc, double* __restrict__ rss,
    double* __restrict__ peak, int32_t* __restrict__ ipeak, double* __restrict__ resid, int64_t resid_stride) {
  typedef double d2v __attribute__((ext_vector_type(2)));
  constexpr int ITS = kResAcc / VEC;      // iterations after which a lane is back at the same t mod 512
  constexpr int UNR = ITS > 4 ? ITS : VEC == 8 ? 2 : 4;  // loads in flight per lane, a multiple of ITS
  constexpr int STEP = 64 * VEC;
  extern __shared__ double res_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const double nan = __builtin_nan("");
  const int64_t s0 = (int64_t)blockIdx.x * kResWaves + wave, ds = (int64_t)gridDim.x * kResWaves;
  for (int64_t sg = s0; sg < nseg; sg += ds) {
    const double a = params[sg], m = params[ld + sg], phi = params[2 * ld + sg], psi = params[3 * ld + sg];
    const double d0 = dc[sg];
    const XT* xs = x + sg * seg_stride;
    double* rs = resid ? resid + sg * resid_stride : nullptr;
    if (!(res_finite(a) && res_finite(m) && res_finite(phi) && res_finite(psi) && res_finite(d0))) {
      if (rs)
        for (int t = lane; t < R; t += 64) rs[t] = nan;
      if (lane == 0) {
        if (rss) rss[sg] = nan;
        if (peak) peak[sg] = nan;
        if (ipeak) ipeak[sg] = -1;
      }
      continue;
    }
    typename std::conditional<PERIODIC, ResPeriodic, ResRotating>::type mdl;
    double part = 0.0;
    if constexpr (PERIODIC) {
      double* A = res_lds + wave * L;
      res_wave_sync();  // the previous segment's table reads are done
      for (int p = lane; p < L; p += 64) {
        const double v = res_ac(a, m, phi, w0 * (double)p + psi);
        A[p] = v;
        const int cnt = p < R ? (R - 1 - p) / L + 1 : 0;
        part = fma((double)cnt, v, part);
      }
      res_wave_sync();
      mdl.A = A;
      mdl.L = L;
      mdl.p = (lane * VEC) % L;
      mdl.dp = STEP % L;
    } else {
      mdl.a = a, mdl.m = m, mdl.phi = phi, mdl.psi = psi, mdl.w0 = w0;
      sincos(w0, &mdl.s1, &mdl.c1);
      sincos(w0 * (double)STEP, &mdl.ss, &mdl.cs);
      for (int tb = 0; tb < R; tb += UNR * STEP) {
        mdl.seek(tb + lane * VEC);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int t = tb + (u * 64 + lane) * VEC;
          double ac[VEC];
          mdl.template next<VEC>(ac);
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            if (t + e < R) part += ac[e];
        }
      }
    }
    const double k = d0 - res_wave_sum(part) / (double)R;
    double acc[kResAcc];
#pragma unroll
    for (int j = 0; j < kResAcc; ++j) acc[j] = 0.0;
    double pk = -1.0;
    int ti = 0x7fffffff;
    for (int tb = 0; tb < R; tb += UNR * STEP) {
      ResRaw<XT, VEC> raw[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) res_load<XT, VEC>(xs, tb + (u * 64 + lane) * VEC, R, raw[u]);
      mdl.seek(tb + lane * VEC);
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int t = tb + (u * 64 + lane) * VEC;
        double ac[VEC], r[VEC];
        mdl.template next<VEC>(ac);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          r[e] = (raw[u].at(e) - k) - ac[e];
          if (t + e < R) {
            double& s2 = acc[(u % ITS) * VEC + e];
            s2 = fma(r[e], r[e], s2);
            const double ar = fabs(r[e]);
            if (ar > pk) {
              pk = ar;
              ti = t + e;
            }
          }
        }
        if (rs) {
          if constexpr (VEC == 1) {
            if (t < R) __builtin_nontemporal_store(r[0], rs + t);
          } else {
#pragma unroll
            for (int e = 0; e < VEC; e += 2) {
              if (t + e + 1 < R) {
                const d2v v = {r[e], r[e + 1]};
                // a lane's VEC doubles leave in VEC / 2 stores: beyond one, a store covers 16 B of every
                // 8 VEC B, and only cached stores merge into whole lines on the way out
                if constexpr (VEC == 2) __builtin_nontemporal_store(v, reinterpret_cast<d2v*>(rs + t + e));
                else *reinterpret_cast<d2v*>(rs + t + e) = v;
              } else if (t + e < R) {
                rs[t + e] = r[e];
              }
            }
          }
        }
      }
    }
    const double tot = res_sum<VEC>(acc);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double po = __shfl_xor(pk, o);
      const int to = __shfl_xor(ti, o);
      if (po > pk || (po == pk && to < ti)) {
        pk = po;
        ti = to;
      }
    }
    if (lane == 0) {
      const bool bad = tot != tot;
      if (rss) rss[sg] = tot;
      if (peak) peak[sg] = bad ? nan : pk;
      if (ipeak) ipeak[sg] = bad ? -1 : ti;
    }
  }
}

// Launch of residual_kernel (residual.hip): L > 0 the periodic evaluator (8 <= L <= kResMaxL),
// L == 0 the rotating one; device pointers; NULL outputs are skipped.
hipError_t residual_launch(const void* x, int xtype, int64_t nseg, int64_t seg_stride, int R, double w0, int L,
                           const double* params, int64_t ld, const double* dc, double* rss, double* peak,
                           int32_t* ipeak, double* resid, int64_t resid_stride, int n_cu, hipStream_t st);

}  // namespace dfmi
