// lpsd.h — point functions of the log-frequency spectral density (dfmi_lpsd):
// the Kaiser window sample, the phasor of a fractional bin and the accumulation of one lane's
// share of a segment. __host__ __device__, so tests/hostcheck_lpsd runs the same code on the
// CPU; lpsd.hip holds the kernels. The pair forms at the end (lpsd_share_bin2, lcsd_coherence)
// are dfmi_lcsd's (host twin tests/hostcheck_lcsd).
//
//   w[n] = I0(pi alpha sqrt(1 - z^2)) / I0(pi alpha), z = 2n/L - 1, n = 0..L-1  (DFT-even Kaiser)
//   alpha = ((0.0889732 p - 0.493285) p + 4.71469) p - 0.0821377, p = psll/100
//   A = sum_n w[n] (x[s+n] - mean) exp(-2 pi i b n / L),  s = floor(k (N-L)/(K-1) + 0.5)
//   Sxx = 2 mean_k |A|^2 / (fs sum w^2),  ENBW = fs sum w^2 / (sum w)^2
//
// I0 is its power series sum (x^2/4)^k / (k!)^2: every term is positive, so the sum carries
// no cancellation. The factors 1/k^2 come from a table the host fills (lpsd_fill_rk2: a
// correctly rounded division each, the same numbers on every build), read at a loop index
// that is uniform over the wave. kLpsdI0Terms terms reach 2^-64 of the sum for every
// argument up to kLpsdI0Max (at x = 64 the terms fall below that from k = 66).
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

constexpr int kLpsdI0Terms = 256;
constexpr double kLpsdI0Max = 64.0;
constexpr double kLpsdPi = 3.141592653589793;
constexpr int64_t kLpsdWaveL = 256;  // segments up to this length: one wave per tile; longer: one workgroup

// One frequency of a call as the kernels read it (sorted longest segment first).
struct LpsdFreq {
  double b;       // fractional bin: the frequency is b fs / L
  int64_t L, K;   // segment length, segment count
  int64_t woff;   // first sample of this frequency's window row in the window workspace
  int64_t toff;   // first of its K tile slots in the tile workspace
  int64_t j;      // index in the caller's plan
};

DFMI_HDI double lpsd_kaiser_alpha(double psll) {
  const double p = psll / 100.0;
  return ((0.0889732 * p - 0.493285) * p + 4.71469) * p - 0.0821377;
}

inline void lpsd_fill_rk2(double* rk2) {
  for (int k = 1; k <= kLpsdI0Terms; ++k) rk2[k - 1] = 1.0 / ((double)k * (double)k);
}

DFMI_HDI double lpsd_i0(double x, const double* __restrict__ rk2) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 0; k < kLpsdI0Terms; ++k) {
    term *= q * rk2[k];
    sum += term;
    if (term < sum * 5.4e-20) break;  // 2^-64 of the sum
  }
  return sum;
}

// Window sample n of a length-L window; pa = pi alpha, inv_i0 = 1 / I0(pa).
DFMI_HDI double lpsd_window(int64_t n, int64_t L, double pa, double inv_i0, const double* __restrict__ rk2) {
  const double z = 2.0 * (double)n / (double)L - 1.0;
  const double r = 1.0 - z * z;
  return lpsd_i0(pa * sqrt(r > 0.0 ? r : 0.0), rk2) * inv_i0;
}

// Start of segment k of K segments of length L in a series of N samples.
DFMI_HDI int64_t lpsd_start(int64_t k, int64_t K, int64_t L, int64_t N) {
  if (K <= 1) return 0;
  int64_t s = (int64_t)floor((double)k * (double)(N - L) / (double)(K - 1) + 0.5);
  if (s < 0) s = 0;
  return s > N - L ? N - L : s;
}

// exp(-2 pi i b n / L) with the phase reduced to one turn first: (c, -s) of 2 pi frac(b n / L).
DFMI_HDI void lpsd_phasor(double b, int64_t n, double L, double* c, double* s) {
  double t = b * (double)n / L;
  t -= floor(t);
  double sn, cs;
  sincos(2.0 * kLpsdPi * t, &sn, &cs);
  *c = cs;
  *s = -sn;
}

// One lane's share of a segment's sum: samples n = lane, lane + team, ... < L.
DFMI_HDI double lpsd_share_sum(const double* __restrict__ x, int64_t L, int lane, int team) {
  double a = 0.0;
  for (int64_t n = lane; n < L; n += team) a += x[n];
  return a;
}

// One lane's share of A = sum w[n] (x[n] - mean) exp(-2 pi i b n / L).
DFMI_HDI void lpsd_share_bin(const double* __restrict__ x, const double* __restrict__ w, int64_t L, double b,
                             double mean, int lane, int team, double* re, double* im) {
  double ar = 0.0, ai = 0.0;
  const double Ld = (double)L;
  for (int64_t n = lane; n < L; n += team) {
    double c, s;
    lpsd_phasor(b, n, Ld, &c, &s);
    const double v = w[n] * (x[n] - mean);
    ar = fma(v, c, ar);
    ai = fma(v, s, ai);
  }
  *re = ar;
  *im = ai;
}

// The pair form (dfmi_lcsd): one lane's share of A (from x, mean mx) and B (from
// y, mean my) with one phasor and one window load per sample. Each accumulator sees the
// expressions of lpsd_share_bin in its order, so A and B are bit for bit what two single calls give.
DFMI_HDI void lpsd_share_bin2(const double* __restrict__ x, const double* __restrict__ y,
                              const double* __restrict__ w, int64_t L, double b, double mx, double my, int lane,
                              int team, double* are, double* aim, double* bre, double* bim) {
  double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
  const double Ld = (double)L;
  for (int64_t n = lane; n < L; n += team) {
    double c, s;
    lpsd_phasor(b, n, Ld, &c, &s);
    const double wn = w[n];
    const double vx = wn * (x[n] - mx);
    const double vy = wn * (y[n] - my);
    ar = fma(vx, c, ar);
    ai = fma(vx, s, ai);
    br = fma(vy, c, br);
    bi = fma(vy, s, bi);
  }
  *are = ar;
  *aim = ai;
  *bre = br;
  *bim = bi;
}

// Magnitude-squared coherence |Sxy|^2 / (Sxx Syy) of one frequency: not clamped (rounding may
// leave it a few 1e-14 above 1); NaN where Sxx Syy is 0 or NaN.
DFMI_HDI double lcsd_coherence(double sxx, double syy, double re, double im) {
  const double den = sxx * syy;
  return den > 0.0 ? fma(re, re, im * im) / den : NAN;
}

}  // namespace dfmi
