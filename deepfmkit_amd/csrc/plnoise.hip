// plnoise.hip — dfmi_plnoise's kernel: ONE WAVE PER SERIES runs plnoise.h's cascade as a
// systolic pipeline, a section per lane.
//
//   gaussians    mt_wave.h's generator; each twisted block's gaussians (at most 312) are
//                staged in LDS in stream order, so the warm-up samples never reach memory
//   pipeline     lane i holds section i's coefficients and state z. At step t it runs sample
//                t - i: its input is lane i - 1's output of step t - 1 (a lane shift), lane 0
//                takes the next gaussian, the last section's lane emits y. Every section
//                sees its samples in order, so each runs plnoise.h's sequential recurrence:
//                the series depends on the gaussians alone. n_warm + n + nsec - 1 steps;
//                lanes outside 0 <= t - i < n_warm + n and lanes >= nsec are masked
//   output       the emitting lane stages scale * y in LDS; the wave writes each block's
//                samples past the warm-up to global memory together
// LDS: 624 state words and 2 x 312 doubles. Built without FMA contraction.
#include <hip/hip_runtime.h>

#include "mt_wave.h"
#include "plnoise.h"

namespace dfmi {
namespace {

constexpr int kStage = 2 * kMtCandidates;  // gaussians of one twisted block, at most

__global__ __launch_bounds__(kMtLanes) void plnoise_wave_kernel(const double* __restrict__ sections, int nsec,
                                                                 double scale, const uint32_t* __restrict__ seeds,
                                                                 double sigma,
                                                                 const dfmi_synth_colour* __restrict__ colour,
                                                                 int64_t n_warm, int64_t n, double* out) {
#pragma clang fp contract(off)
  __shared__ uint32_t mt[kMtN];
  __shared__ double stage[kStage];
  __shared__ double ostage[kStage];
  const int64_t r = blockIdx.x;
  const int lane = threadIdx.x;
  uint32_t seed;
  if (colour) {
    const dfmi_synth_colour c = colour[r];
    if (c.g_freq == 0.0 && c.g_arm == 0.0) return;  // no coloured source: no basis is read
    seed = c.seed;
    sigma = c.sigma;
  } else {
    seed = seeds[r];
  }
  const bool live = lane < nsec;
  const double a0 = live ? sections[3 * lane] : 0.0;
  const double a1 = live ? sections[3 * lane + 1] : 0.0;
  const double b1 = live ? sections[3 * lane + 2] : 0.0;
  const int64_t T = n_warm + n, total = T + (nsec - 1);
  double* o = out + r * n;
  double z = 0.0, y = 0.0;  // y: this lane's output of the previous step

  mt_wave_seed(mt, seed, lane);
  int64_t t0 = 0;
  while (t0 < total) {
    const bool feeding = t0 < T;
    int cnt;
    if (feeding) {
      mt_wave_twist(mt, lane);
      int g = 0;
      for (int c0 = 0; c0 < kMtCandidates; c0 += kMtLanes) {
        const int base = g;
        g += mt_wave_polar(mt, c0, lane, [=](int rel, double g0, double g1) {
          stage[base + rel] = g0;
          stage[base + rel + 1] = g1;
        });
      }
      __syncthreads();
      cnt = (int64_t)g < T - t0 ? g : (int)(T - t0);
    } else {
      cnt = (int)(total - t0);  // the drain: nsec - 1 steps without input
    }
    for (int s = 0; s < cnt; ++s) {
      double x = __shfl_up(y, 1);
      if (lane == 0) x = feeding ? 0.0 + sigma * stage[s] : 0.0;
      const int64_t k = t0 + s - lane;  // this lane's sample
      if (live && k >= 0 && k < T) y = pl_step(a0, a1, b1, x, &z);
      if (lane == nsec - 1) ostage[s] = scale * y;
    }
    __syncthreads();
    // step t0 + s emitted sample t0 + s - (nsec - 1); those past the warm-up are the series
    for (int s = lane; s < cnt; s += kMtLanes) {
      const int64_t e = t0 + s - (nsec - 1) - n_warm;
      if (e >= 0 && e < n) o[e] = ostage[s];
    }
    __syncthreads();
    t0 += cnt;
  }
}

}  // namespace

hipError_t plnoise_launch(const double* d_sections, int nsec, double scale, const uint32_t* d_seeds, double sigma,
                          const dfmi_synth_colour* d_colour, int64_t nser, int64_t n_warm, int64_t n, double* out,
                          hipStream_t st) {
  if (nser == 0) return hipSuccess;
  hipLaunchKernelGGL(plnoise_wave_kernel, dim3((unsigned)nser), dim3(kMtLanes), 0, st, d_sections, nsec, scale,
                     d_seeds, sigma, d_colour, n_warm, n, out);
  return hipGetLastError();
}

}  // namespace dfmi
