// plnoise_design.cpp — dfmi_plnoise_design: the C entry of the host-only section table
// (plnoise_design.h). Compiled by the host compiler, beside lpsd_plan.cpp: no device
// code, no fast-math.
#include "../../include/dfmi.h"
#include "plnoise_design.h"

extern "C" int dfmi_plnoise_design(double fs, int64_t n, double alpha, double* sections, int32_t cap, double* scale) {
  if (sections && cap < 0) return DFMI_ERR_ARG;
  const int nsec = dfmi::pl_design(fs, n, alpha, sections, cap, scale);
  return nsec == -2 ? DFMI_ERR_UNSUPPORTED : nsec < 0 ? DFMI_ERR_ARG : nsec;
}
