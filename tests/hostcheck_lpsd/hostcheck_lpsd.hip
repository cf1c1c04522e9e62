// hostcheck_lpsd.hip — TEST-ONLY host build of deepfmkit_amd/csrc/lpsd.h (the point functions
// dfmi_lpsd's kernels run per lane) and csrc/lpsd_plan.h, so the CPU suite can gate the
// window, the plan and the estimate without a GPU. The lanes of a team are walked in turn
// and their partial sums are combined in the kernels' order (the shuffle tree of a wave, then
// the four waves in turn). The product library never links this; tests/test_gpu_lpsd.py
// exercises the real kernels.
#include <vector>

#include "../../deepfmkit_amd/csrc/lpsd.h"
#include "../../deepfmkit_amd/csrc/lpsd_plan.h"

namespace {

// lpsd.hip wave_sum: lane 0 of a shuffle-down tree over 64 lanes
double wave_sum(double* v) {
  for (int o = 32; o > 0; o >>= 1)
    for (int i = 0; i < o; ++i) v[i] += v[i + o];
  return v[0];
}

// lpsd.hip team_sum over `team` lanes (64 or 256)
double team_sum(std::vector<double>& v, int team) {
  if (team == 64) return wave_sum(v.data());
  double w[4];
  for (int i = 0; i < 4; ++i) w[i] = wave_sum(v.data() + 64 * i);
  return ((w[0] + w[1]) + w[2]) + w[3];
}

}  // namespace

extern "C" {

double hc_lpsd_alpha(double psll) { return dfmi::lpsd_kaiser_alpha(psll); }

// w[0..L) and sums[0] = sum w, sums[1] = sum w^2 in lpsd_wsum_kernel's order
void hc_lpsd_window(int64_t L, double psll, double* w, double* sums) {
  double rk2[dfmi::kLpsdI0Terms];
  dfmi::lpsd_fill_rk2(rk2);
  const double pa = dfmi::kLpsdPi * dfmi::lpsd_kaiser_alpha(psll);
  const double inv_i0 = 1.0 / dfmi::lpsd_i0(pa, rk2);
  for (int64_t n = 0; n < L; ++n) w[n] = dfmi::lpsd_window(n, L, pa, inv_i0, rk2);
  std::vector<double> s1(256, 0.0), s2(256, 0.0);
  for (int l = 0; l < 256; ++l)
    for (int64_t n = l; n < L; n += 256) {
      s1[l] += w[n];
      s2[l] = fma(w[n], w[n], s2[l]);
    }
  sums[0] = team_sum(s1, 256);
  sums[1] = team_sum(s2, 256);
}

int64_t hc_lpsd_plan(int64_t N, double fs, double olap, double bmin, int64_t Lmin, int64_t Jdes, int64_t Kdes,
                     double* f, double* fres, double* b, int64_t* L, int64_t* K, int64_t cap) {
  return dfmi::lpsd_plan(N, fs, olap, bmin, Lmin, Jdes, Kdes, f, fres, b, L, K, cap);
}

// dfmi_lpsd's arithmetic: Sxx[r*J + j], enbw[j]
void hc_lpsd(const double* x, int64_t nser, int64_t ser_stride, int64_t N, double fs, const double* b, const int64_t* L,
             const int64_t* K, int64_t J, int32_t order, double psll, double* Sxx, double* enbw) {
  std::vector<double> w, a(256), re(256), im(256), part(256);
  for (int64_t j = 0; j < J; ++j) {
    w.resize((size_t)L[j]);
    double sums[2];
    hc_lpsd_window(L[j], psll, w.data(), sums);
    const int team = L[j] > dfmi::kLpsdWaveL ? 256 : 64;
    enbw[j] = fs * sums[1] / (sums[0] * sums[0]);
    for (int64_t r = 0; r < nser; ++r) {
      for (int l = 0; l < 256; ++l) part[l] = 0.0;
      for (int64_t k = 0; k < K[j]; ++k) {
        const double* xs = x + r * ser_stride + dfmi::lpsd_start(k, K[j], L[j], N);
        double mean = 0.0;
        if (order == 0) {
          for (int l = 0; l < team; ++l) a[l] = dfmi::lpsd_share_sum(xs, L[j], l, team);
          mean = team_sum(a, team) / (double)L[j];
        }
        for (int l = 0; l < team; ++l) dfmi::lpsd_share_bin(xs, w.data(), L[j], b[j], mean, l, team, &re[l], &im[l]);
        const double ar = team_sum(re, team), ai = team_sum(im, team);
        part[k % 256] += ar * ar + ai * ai;  // lpsd_finish_kernel: lane k % 256 adds tile k
      }
      Sxx[r * J + j] = 2.0 * (team_sum(part, 256) / (double)K[j]) / (fs * sums[1]);
    }
  }
}

}  // extern "C"
