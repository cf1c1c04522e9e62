// plnoise_design.h — the section table of plnoise.h's cascade: host only, plain C++ (the
// host compiler builds it into dfmi_plnoise_design, the test-only host build calls it too).
#pragma once
#include <math.h>
#include <stdint.h>

namespace dfmi {

constexpr int kPlMaxSections = 64;  // one section per lane of a wave (plnoise.hip)

// The section table of (fs, n, alpha): sections[3 i + (0, 1, 2)] = a0, a1, b1 of section i,
// *scale = f_max^(-alpha / 2). Returns nsec; -1 for arguments outside n >= 4, fs > 0 and
// finite, 0 < alpha <= 2; -2 where nsec > kPlMaxSections. sections == NULL only counts;
// otherwise cap >= nsec entries are required (-1 when there is less room).
inline int pl_design(double fs, int64_t n, double alpha, double* sections, int cap, double* scale) {
#pragma clang fp contract(off)
  if (n < 4 || !(fs > 0.0) || !(fs <= 1.7976931348623157e308) || !(alpha > 0.0) || !(alpha <= 2.0)) return -1;
  const double pi = 3.141592653589793;
  const double f_min = fs / (double)n, f_max = fs / 2.0;
  const double lw0 = log10(2.0 * pi * f_min), lw1 = log10(2.0 * pi * f_max);
  const double span = lw1 - lw0;
  const double cnt = ceil(4.5 * span);
  if (!(cnt >= 1.0)) return -1;
  if (cnt > (double)kPlMaxSections) return -2;
  const int nsec = (int)cnt;
  if (scale) *scale = pow(f_max, -alpha / 2.0);
  if (!sections) return nsec;
  if (cap < nsec) return -1;
  const double dp = span / (double)nsec;
  for (int i = 0; i < nsec; ++i) {
    const double lp = lw0 + dp * 0.5 * ((double)(2 * i + 1) - alpha / 2.0);
    const double f0 = pow(10.0, lp) / (2.0 * pi);
    const double f1 = pow(10.0, lp + dp * alpha / 2.0) / (2.0 * pi);
    const double den = fs + pi * f0;
    sections[3 * i] = (fs + pi * f1) / den;
    sections[3 * i + 1] = -(fs - pi * f1) / den;
    sections[3 * i + 2] = (fs - pi * f0) / den;
  }
  return nsec;
}

}  // namespace dfmi
