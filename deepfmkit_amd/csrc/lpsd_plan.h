// lpsd_plan.h — the frequency plan of the log-frequency spectral density (dfmi_lpsd_plan):
// which Fourier frequencies are estimated, and with which segment length L, segment count K
// and (fractional) bin b each. Plain C++, host only, all arithmetic double; the definition is
// DESIGN.md §13 (after Tröbs & Heinzel 2006 and LTPDA's ltf_plan) and is restated in numpy by
// tests/helpers/lpsd_ref.py.
//
//   xov = 1 - olap, fresmin = fs/N, freslim = fresmin (1 + xov (Kdes - 1)),
//   logfact = (N/2)^(1/Jdes) - 1; fi = fresmin bmin; while fi < fs/2:
//     fres = fi logfact; fres <= freslim: fres = sqrt(fres freslim); fres < fresmin: fres = fresmin
//     b = fi/fres; b < bmin: b = bmin, fres = fi/b
//     L = floor(fs/fres + 0.5) within [max(Lmin, 1), N]; K = floor((N-L)/(xov L) + 1 + 0.5);
//     K == 1: L = N;  fres = fs/L, b = fi/fres;
//     bin floor: if that b < bmin (the rounding of L moves it by up to fi/(2 fs)), L becomes the
//       shortest length with fi L / fs >= bmin, at most N, and K, fres, b are formed again
//     emit (fi, fres, b, L, K);  fi += fres
// so every emitted b >= bmin. Without the floor this is LTPDA's loop, whose b can end below
// bmin; plans in which it never does are unchanged by it (every default-setting plan is).
#pragma once
#include <math.h>
#include <stdint.h>

namespace dfmi {

// Writes at most `cap` entries when the output pointers are given (all five or none) and
// returns J, the number of frequencies of the plan; -1 for a rejected argument, -2 when J
// exceeds cap.
inline int64_t lpsd_plan(int64_t N, double fs, double olap, double bmin, int64_t Lmin, int64_t Jdes, int64_t Kdes,
                         double* f, double* fres_out, double* b_out, int64_t* L_out, int64_t* K_out, int64_t cap) {
  if (N < 8 || !(fs > 0.0) || !(fs <= 1.7976931348623157e308) || !(olap >= 0.0 && olap < 1.0) ||
      !(bmin > 0.0 && bmin <= 1.7976931348623157e308) || Jdes < 1 || Kdes < 1)
    return -1;
  const bool write = f && fres_out && b_out && L_out && K_out;
  const double xov = 1.0 - olap;
  const double fresmin = fs / (double)N;
  const double freslim = fresmin * (1.0 + xov * (double)(Kdes - 1));
  const double logfact = pow((double)N / 2.0, 1.0 / (double)Jdes) - 1.0;
  const int64_t lmin = Lmin > 1 ? Lmin : 1;
  int64_t J = 0;
  double fi = fresmin * bmin;
  while (fi < fs / 2.0) {
    double fres = fi * logfact;
    if (fres <= freslim) fres = sqrt(fres * freslim);
    if (fres < fresmin) fres = fresmin;
    double b = fi / fres;
    if (b < bmin) {
      b = bmin;
      fres = fi / b;
    }
    const double Ld = floor(fs / fres + 0.5);
    int64_t L = Ld >= (double)N ? N : (int64_t)Ld;
    if (L < lmin) L = lmin;
    if (L > N) L = N;
    int64_t K = (int64_t)floor((double)(N - L) / (xov * (double)L) + 1.0 + 0.5);
    if (K == 1) L = N;
    fres = fs / (double)L;
    b = fi / fres;
    if (b < bmin) {
      // the bin floor: rounding L moved b = fi L / fs below bmin (by up to fi / (2 fs)); take
      // the shortest segment that keeps it (at most N: fi >= bmin fs / N), and K, fres, b again
      const double Lf = ceil(bmin * fs / fi);
      L = Lf >= (double)N ? N : (int64_t)Lf;
      if (L < lmin) L = lmin;
      while (fi / (fs / (double)L) < bmin && L < N) ++L;
      K = (int64_t)floor((double)(N - L) / (xov * (double)L) + 1.0 + 0.5);
      if (K == 1) L = N;
      fres = fs / (double)L;
      b = fi / fres;
      if (b < bmin) b = bmin;  // L = N and fi = fresmin bmin: b is bmin but for the quotient's rounding
    }
    if (write) {
      if (J >= cap) return -2;
      f[J] = fi;
      fres_out[J] = fres;
      b_out[J] = b;
      L_out[J] = L;
      K_out[J] = K;
    }
    ++J;
    fi += fres;  // fres >= fs/N > 0: at most N/2 + 1 steps
  }
  return J;
}

}  // namespace dfmi
