// plnoise.h — coloured (1/f^alpha) noise: the pole-zero cascade of Plaszczynski (2007),
// the project's own definition (pyplnoise parity is not pinned).
//
//   design   nsec first-order sections spaced evenly in log10(omega) between
//            2 pi fs/N and 2 pi fs/2, each (a0, a1, b1) of the bilinear pole-zero pair
//   series   x = RandomState(seed).normal(scale = sigma, size = n_warm + n); every section
//            in turn, zero initial state:  y[k] = a0 x[k] + z,  z = a1 x[k] + b1 y[k]
//            (scipy.signal.lfilter([a0, a1], [1, -b1], x) bit for bit); the section's y is
//            the next section's x;  basis = scale * y[n_warm:]
// Every function rounds operation by operation (no FMA contraction, whatever the
// translation unit's flags), so the series depends on the gaussians alone.
#pragma once
#include <math.h>
#include <stdint.h>

#include "plnoise_design.h"
#include "synth.h"

namespace dfmi {

// One sample through one section (direct form II transposed): returns y, updates z
DFMI_SY_HD double pl_step(double a0, double a1, double b1, double x, double* z) {
#pragma clang fp contract(off)
  const double y = a0 * x + *z;
  *z = a1 * x + b1 * y;
  return y;
}

// The whole cascade over v(0..T) in place, section by section (the sequential order)
template <typename Vec>
DFMI_SY_HD void pl_cascade(const double* sections, int nsec, int64_t T, Vec v) {
  for (int i = 0; i < nsec; ++i) {
    const double a0 = sections[3 * i], a1 = sections[3 * i + 1], b1 = sections[3 * i + 2];
    double z = 0.0;
    for (int64_t k = 0; k < T; ++k) v(k) = pl_step(a0, a1, b1, v(k), &z);
  }
}

// One series: work(0..n_warm + n) is scratch, out(0..n) = scale * y[n_warm:]
template <typename Key, typename Vec, typename Out>
DFMI_SY_HD void pl_series(const double* sections, int nsec, double scale, double sigma, uint32_t seed,
                          int64_t n_warm, int64_t n, Key key, Vec work, Out out) {
#pragma clang fp contract(off)
  Mt<Key> mt{key, 0, false, 0.0};
  mt.seed(seed);
  const int64_t T = n_warm + n;
  for (int64_t k = 0; k < T; ++k) work(k) = 0.0 + sigma * mt.next_gauss();
  pl_cascade(sections, nsec, T, work);
  for (int64_t k = 0; k < n; ++k) out(k) = scale * work(n_warm + k);
}

#if defined(__HIPCC__)
// plnoise.hip: one wave per series. seeds (device, nser) with one sigma, or colour (device,
// nser rows: seed and sigma per series; a row whose gains are both 0 is skipped).
hipError_t plnoise_launch(const double* d_sections, int nsec, double scale, const uint32_t* d_seeds, double sigma,
                          const dfmi_synth_colour* d_colour, int64_t nser, int64_t n_warm, int64_t n, double* out,
                          hipStream_t st);
#endif

}  // namespace dfmi
