// demod_window.h — demodulation under a cosine-sum window (Hann, Hamming, Blackman,
// Blackman-Harris) folded into the fold kernel's phase bins.
//
// Definition (include/dfmi.h dfmi_demod_window): w[t] = Σ_{m<=K} a_m cos(2π m t / R), t < R,
//     Q_h = Σ_t w[t] x[t] cos(ω_h t) / Σ_t w[t],   I_h with sin,   dc = Σ w x / Σ w,
// ω_h = fl(h·w0) and Σ w = R·a_0 for R > K.
//
// No per-sample weight table. With the basis periodic in L samples and t = p + k·L (phase bin p,
// cycle k), angle addition splits every cosine of the window into a per-bin and a per-cycle factor:
//     cos(2π m (p + k L) / R) = cos(β_m p)·c_{m,k} − sin(β_m p)·s_{m,k},    β_m = 2π m / R,
//     c_{m,k} = cos(β_m k L), s_{m,k} = sin(β_m k L).
// c and s are the same for every bin of cycle k, so the windowed fold is 1 + 2K plain folds with
// wave-uniform weights,
//     A[p] = Σ_k x[p + kL],   B_m[p] = Σ_k x[p + kL]·c_{m,k},   C_m[p] = Σ_k x[p + kL]·s_{m,k},
// and the windowed bins follow once per segment by one small rotation per bin,
//     y[p] = A[p] + Σ_m (a_m / a_0)·(cos(β_m p)·B_m[p] − sin(β_m p)·C_m[p]),
// after which fold_finish (demod.h) contracts y with the basis exactly as for the rectangular
// window: its division by R is Σ w / a_0. 1 + 2K FMAs per sample (3 for Hann), so the kernel stays a
// stream of the samples. The algebra holds for any R: a ragged last cycle (R not a multiple of L)
// is cycle ncyc with element-wise bounds.
//
// Mapping: fold_segment's. One wave owns one segment at a time (persistent grid-stride over
// 4-wave workgroups), lane l owns the bins p = VEC·(l + 64·j) + e, a cycle is MAXSLOT coalesced
// wave loads and 8 loads stay in flight per lane. The per-cycle weights (wcyc: cycle k's
// c_1..c_K, s_1..s_K, ceil(R / L) cycles) are read through wave-uniform addresses, i.e. by scalar
// loads into SGPRs that the FMAs take as operands. The per-bin factors (wbin: rows
// (a_m/a_0)·cos(β_m p), m = 1..K, then the sin rows, L entries each) belong to fixed lanes: a wave
// loads its own once and keeps them in registers over all its segments (2K·MAXSLOT·VEC doubles),
// except at MAXSLOT 4 with K >= 2, where they would push the kernel towards spilling and are read
// from LDS at the finish instead (FAC_LDS). The basis table sits in LDS, shared by the workgroup.
// Both tables are formed on the host in long double from exactly reduced arguments (m·k·L mod R
// and m·p mod R) and rounded once.
#pragma once
#include "demod.h"

namespace dfmi {

constexpr int kWinLoads = 8;  // vector loads in flight per lane in the fold loop, as fold_segment

template <int MAXSLOT, int K>
constexpr bool win_fac_lds() {
  return MAXSLOT >= 4 && K >= 2;
}

// One cycle's samples v into the 1 + 2K accumulator sets; cw: the cycle's 2K weights (wave-uniform).
template <int VEC, int MAXSLOT, int K>
__device__ __forceinline__ void win_add(double (&acc)[1 + 2 * K][MAXSLOT][VEC], const double (&v)[MAXSLOT][VEC],
                                        const double* __restrict__ cw) {
  double w[2 * K];
#pragma unroll
  for (int m = 0; m < 2 * K; ++m) w[m] = cw[m];
#pragma unroll
  for (int j = 0; j < MAXSLOT; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[0][j][e] += v[j][e];
#pragma unroll
      for (int m = 0; m < 2 * K; ++m) acc[1 + m][j][e] = fma(v[j][e], w[m], acc[1 + m][j][e]);
    }
}

template <int VEC, int MAXSLOT, int K, typename XT>
__global__ __launch_bounds__(kBlockThreads) void demod_window_kernel(
    const XT* __restrict__ x, int64_t nseg, int64_t seg_stride, int R, int L, int ndata,
    const double* __restrict__ tab, const double* __restrict__ wcyc, const double* __restrict__ wbin,
    double* __restrict__ qi, int64_t qi_ld, double* __restrict__ dc) {
  constexpr bool FAC_LDS = win_fac_lds<MAXSLOT, K>();
  constexpr int UNR = (MAXSLOT >= kWinLoads) ? 1 : (kWinLoads / MAXSLOT);
  extern __shared__ __attribute__((aligned(16))) double lds_win[];  // basis [2 ndata][L] | FAC_LDS: wbin [2K][L]
  const int ntab = 2 * ndata * L;  // even: the factors behind it stay 16-B aligned
  stage_table(tab, lds_win, ntab, threadIdx.x, kBlockThreads);
  if constexpr (FAC_LDS) stage_table(wbin, lds_win + ntab, 2 * K * L, threadIdx.x, kBlockThreads);
  __syncthreads();
  const double* __restrict__ F = lds_win + ntab;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nslot = (L + 64 * VEC - 1) / (64 * VEC);
  const int ncyc = R / L;
  const int rem = R - ncyc * L;
  int pbase[MAXSLOT];
  bool pval[MAXSLOT];
#pragma unroll
  for (int j = 0; j < MAXSLOT; ++j) {
    pbase[j] = VEC * (lane + 64 * j);
    pval[j] = (j < nslot) && (pbase[j] < L);
  }
  // this lane's per-bin factors, for all its segments
  double fac[FAC_LDS ? 1 : 2 * K][MAXSLOT][VEC];
  if constexpr (!FAC_LDS) {
#pragma unroll
    for (int m = 0; m < 2 * K; ++m)
#pragma unroll
      for (int j = 0; j < MAXSLOT; ++j) {
        if (pval[j]) VecT<VEC>::load(wbin + m * L + pbase[j], fac[m][j]);
        else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) fac[m][j][e] = 0.0;
        }
      }
  }

  for (int64_t s = (int64_t)blockIdx.x * kWavesPerBlock + wave; s < nseg;
       s += (int64_t)gridDim.x * kWavesPerBlock) {
    const XT* __restrict__ xs = x + s * seg_stride;
    double acc[1 + 2 * K][MAXSLOT][VEC];
#pragma unroll
    for (int a = 0; a < 1 + 2 * K; ++a)
#pragma unroll
      for (int j = 0; j < MAXSLOT; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[a][j][e] = 0.0;

    // ---- fold: the full cycles, UNR of them (kWinLoads loads) in flight ----
    int k = 0;
    for (; k + UNR <= ncyc; k += UNR) {
      double v[UNR][MAXSLOT][VEC];
#pragma unroll
      for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int j = 0; j < MAXSLOT; ++j) {
          if (pval[j]) SampleT<XT>::template load_nt<VEC>(xs + (int64_t)(k + u) * L + pbase[j], v[u][j]);
          else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[u][j][e] = 0.0;
          }
        }
#pragma unroll
      for (int u = 0; u < UNR; ++u) win_add<VEC, MAXSLOT, K>(acc, v[u], wcyc + (k + u) * 2 * K);
    }
    for (; k < ncyc; ++k) {
      double v[MAXSLOT][VEC];
#pragma unroll
      for (int j = 0; j < MAXSLOT; ++j) {
        if (pval[j]) SampleT<XT>::template load<VEC>(xs + (int64_t)k * L + pbase[j], v[j]);
        else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) v[j][e] = 0.0;
        }
      }
      win_add<VEC, MAXSLOT, K>(acc, v, wcyc + k * 2 * K);
    }
    if (rem) {  // ragged last cycle: its own weights, element-wise bounds
      const XT* xr = xs + (int64_t)ncyc * L;
      double v[MAXSLOT][VEC];
#pragma unroll
      for (int j = 0; j < MAXSLOT; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          v[j][e] = (pval[j] && pbase[j] + e < rem) ? SampleT<XT>::at(xr + (pbase[j] + e)) : 0.0;
      win_add<VEC, MAXSLOT, K>(acc, v, wcyc + ncyc * 2 * K);
    }

    // ---- finish: one rotation per bin, then the rectangular kernel's contraction ----
    double y[MAXSLOT][VEC];
#pragma unroll
    for (int j = 0; j < MAXSLOT; ++j) {
      double fc[K][VEC], fs[K][VEC];
#pragma unroll
      for (int m = 0; m < K; ++m) {
        if constexpr (FAC_LDS) {
          if (pval[j]) {
            VecT<VEC>::load(F + m * L + pbase[j], fc[m]);
            VecT<VEC>::load(F + (K + m) * L + pbase[j], fs[m]);
          } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) fc[m][e] = fs[m][e] = 0.0;
          }
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            fc[m][e] = fac[m][j][e];
            fs[m][e] = fac[K + m][j][e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        double t = acc[0][j][e];
#pragma unroll
        for (int m = 0; m < K; ++m) {
          t = fma(fc[m][e], acc[1 + m][j][e], t);
          t = fma(-fs[m][e], acc[1 + K + m][j][e], t);
        }
        y[j][e] = t;
      }
    }
    fold_finish<VEC, MAXSLOT>(y, pval, pbase, R, L, ndata, lds_win, lane, qi, qi_ld, s, dc);
  }
}

}  // namespace dfmi
