// hostcheck_lcsd.hip — TEST-ONLY host build of the pair forms in deepfmkit_amd/csrc/lpsd.h
// (lpsd_share_bin2, lcsd_coherence: what dfmi_lcsd's kernels run per lane), so the CPU suite can
// gate the cross-spectral density and the coherence without a GPU. The lanes of a team are
// walked in turn and their partial sums combined in the kernels' order, with the window and
// the team sums of tests/hostcheck_lpsd (its source is included: one statement of them). The
// product library never links this; tests/test_gpu_lcsd.py exercises the real kernels.
#include "../hostcheck_lpsd/hostcheck_lpsd.hip"

extern "C" {

// dfmi_lcsd's arithmetic: out[p*J + j] for every output that is not NULL, enbw[j]
void hc_lcsd(const double* x, int64_t x_stride, const double* y, int64_t y_stride, int64_t npair, int64_t N, double fs,
             const double* b, const int64_t* L, const int64_t* K, int64_t J, int32_t order, double psll, double* Sxx,
             double* Syy, double* Sxy_re, double* Sxy_im, double* coh, double* enbw) {
  std::vector<double> w, a(256), ar(256), ai(256), br(256), bi(256), part[4];
  for (int q = 0; q < 4; ++q) part[q].resize(256);
  for (int64_t j = 0; j < J; ++j) {
    w.resize((size_t)L[j]);
    double sums[2];
    hc_lpsd_window(L[j], psll, w.data(), sums);
    const int team = L[j] > dfmi::kLpsdWaveL ? 256 : 64;
    if (enbw) enbw[j] = fs * sums[1] / (sums[0] * sums[0]);
    for (int64_t p = 0; p < npair; ++p) {
      for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 256; ++l) part[q][l] = 0.0;
      for (int64_t k = 0; k < K[j]; ++k) {
        const int64_t s = dfmi::lpsd_start(k, K[j], L[j], N);
        const double *xs = x + p * x_stride + s, *ys = y + p * y_stride + s;
        double mx = 0.0, my = 0.0;
        if (order == 0) {
          for (int l = 0; l < team; ++l) a[l] = dfmi::lpsd_share_sum(xs, L[j], l, team);
          mx = team_sum(a, team) / (double)L[j];
          for (int l = 0; l < team; ++l) a[l] = dfmi::lpsd_share_sum(ys, L[j], l, team);
          my = team_sum(a, team) / (double)L[j];
        }
        for (int l = 0; l < team; ++l)
          dfmi::lpsd_share_bin2(xs, ys, w.data(), L[j], b[j], mx, my, l, team, &ar[l], &ai[l], &br[l], &bi[l]);
        const double Ar = team_sum(ar, team), Ai = team_sum(ai, team);
        const double Br = team_sum(br, team), Bi = team_sum(bi, team);
        // lcsd_finish_kernel: lane k % 256 adds tile k of each plane
        part[0][k % 256] += Ar * Ar + Ai * Ai;
        part[1][k % 256] += Br * Br + Bi * Bi;
        part[2][k % 256] += Ar * Br + Ai * Bi;
        part[3][k % 256] += Ar * Bi - Ai * Br;
      }
      double v[4];
      for (int q = 0; q < 4; ++q) v[q] = 2.0 * (team_sum(part[q], 256) / (double)K[j]) / (fs * sums[1]);
      const int64_t o = p * J + j;
      if (Sxx) Sxx[o] = v[0];
      if (Syy) Syy[o] = v[1];
      if (Sxy_re) Sxy_re[o] = v[2];
      if (Sxy_im) Sxy_im[o] = v[3];
      if (coh) coh[o] = dfmi::lcsd_coherence(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // extern "C"
