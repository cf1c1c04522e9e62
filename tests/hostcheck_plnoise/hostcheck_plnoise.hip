// hostcheck_plnoise.hip — TEST-ONLY host build of deepfmkit_amd/csrc/plnoise.h (the section
// step and cascade dfmi_plnoise's kernel runs per lane), plnoise_design.h and the coloured
// trial of synth.h, so the CPU suite can gate the design, the cascade and whole coloured
// asd-mode trials without a GPU (host libm log / cos / sin, numpy's own). The product
// library never links this; tests/test_gpu_plnoise.py exercises the real kernel.
#include <vector>

#include "../../deepfmkit_amd/csrc/plnoise.h"

namespace {
struct HKey {
  uint32_t* p;
  uint32_t& operator()(int i) const { return p[i]; }
};
struct HVec {
  double* p;
  double& operator()(int64_t k) const { return p[k]; }
};
}  // namespace

extern "C" {

int hc_plnoise_design(double fs, int64_t n, double alpha, double* sections, int cap, double* scale) {
  return dfmi::pl_design(fs, n, alpha, sections, cap, scale);
}

// one series: out[0..n) = scale * y[n_warm:]
void hc_plnoise(const double* sections, int nsec, double scale, double sigma, uint32_t seed, int64_t n_warm, int64_t n,
                double* out) {
  std::vector<uint32_t> key(dfmi::kMtN);
  std::vector<double> work((size_t)(n_warm + n));
  dfmi::pl_series(sections, nsec, scale, sigma, seed, n_warm, n, HKey{key.data()}, HVec{work.data()}, HVec{out});
}

int64_t hc_sizeof_synth_colour(void) { return (int64_t)sizeof(dfmi_synth_colour); }

// a whole asd-mode trial with the coloured sources of `c` (c == NULL: synth_trial itself)
void hc_synth_trial_coloured(const dfmi_synth_trial* p, const dfmi_synth_colour* c, const double* sections, int nsec,
                             double scale, int64_t n_warm, int64_t n, double f_samp, double* out) {
  std::vector<uint32_t> key(dfmi::kMtN);
  std::vector<double> a(n), d(n), ph(n), basis(n, 0.0);
  if (!c) {
    dfmi::synth_trial(*p, n, f_samp, HKey{key.data()}, HVec{a.data()}, HVec{d.data()}, HVec{ph.data()}, HVec{out});
    return;
  }
  if (c->g_freq != 0.0 || c->g_arm != 0.0)
    hc_plnoise(sections, nsec, scale, c->sigma, c->seed, n_warm, n, basis.data());
  dfmi::synth_trial_coloured(*p, *c, n, f_samp, HKey{key.data()}, HVec{a.data()}, HVec{d.data()}, HVec{ph.data()},
                             HVec{basis.data()}, HVec{out});
}

}  // extern "C"
