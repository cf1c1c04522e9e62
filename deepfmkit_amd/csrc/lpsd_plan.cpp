// lpsd_plan.cpp — dfmi_lpsd_plan: the C entry of the host-only frequency plan (lpsd_plan.h).
// Compiled by the host compiler, beside textio.cpp: no device code, no fast-math.
#include "../../include/dfmi.h"
#include "lpsd_plan.h"

extern "C" int64_t dfmi_lpsd_plan(int64_t N, double fs, double olap, double bmin, int64_t Lmin, int64_t Jdes,
                                  int64_t Kdes, double* f, double* fres, double* b, int64_t* L, int64_t* K,
                                  int64_t cap) {
  const bool any = f || fres || b || L || K, all = f && fres && b && L && K;
  if (any && (!all || cap < 0)) return DFMI_ERR_ARG;
  const int64_t J = dfmi::lpsd_plan(N, fs, olap, bmin, Lmin, Jdes, Kdes, f, fres, b, L, K, cap);
  return J < 0 ? DFMI_ERR_ARG : J;
}
