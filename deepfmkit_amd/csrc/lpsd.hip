// lpsd.hip — dfmi_lpsd's kernels (point functions: lpsd.h; definition: DESIGN.md §13).
//
//   lpsd_window_kernel  fills the window row of every frequency of a batch (grid.y = frequency)
//   lpsd_wsum_kernel    sum w and sum w^2 of each row, one workgroup per frequency
//   lpsd_tile_kernel    one (frequency, segment) tile per team: the segment's mean, then its
//                       windowed bin; |A|^2 goes to the tile workspace. TEAM = 256: one
//                       workgroup per tile (partials reduced in each wave, then through LDS);
//                       TEAM = 64: one wave per tile, four tiles per workgroup, no LDS
//   lpsd_finish_kernel  sums each frequency's K tile values and writes Sxx and ENBW
//   lcsd_tile_kernel,   dfmi_lcsd's pair forms: A of x and B of y from one phasor
//   lcsd_finish_kernel  per sample, four values per tile; Sxx, Syy, Sxy, coherence and ENBW
// The frequencies arrive sorted longest segment first, so the tiles of a launch are ordered
// heaviest first. Every sum has a fixed order (a lane's stride, the shuffle tree, the four
// waves in turn): no atomics, and results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include "lpsd.h"

namespace dfmi {

namespace {

// Sum over the wave, in every lane.
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return __shfl(v, 0, 64);
}

// Sum over a 256-lane workgroup, in every lane: waves 0..3 in turn. Every lane of the
// workgroup must call it.
__device__ __forceinline__ double block_sum(double v, double* lds) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return r;
}

template <int TEAM>
__device__ __forceinline__ double team_sum(double v, double* lds) {
  if constexpr (TEAM == 64) return wave_sum(v);
  else return block_sum(v, lds);
}

// The tile of this team among the ntiles slots [fr[0].toff, ...) of a launch's nf frequencies:
// its slot and frequency. False past the last tile: a whole team leaves together (TEAM = 256:
// the whole workgroup). lpsd_tile_kernel spells the same search out: routed through here its
// instructions come out in another order, and dfmi_lpsd's code objects stay byte for byte what
// they were (scripts/kernel_resources.py --hash).
template <int TEAM>
__device__ __forceinline__ bool team_tile(const LpsdFreq* __restrict__ fr, int nf, int64_t ntiles, LpsdFreq* F,
                                          int64_t* slot) {
  constexpr int kTilesPerBlock = 256 / TEAM;
  const int64_t t = (int64_t)blockIdx.x * kTilesPerBlock + (TEAM == 64 ? (int)(threadIdx.x >> 6) : 0);
  if (t >= ntiles) return false;
  *slot = fr[0].toff + t;
  int lo = 0, hi = nf - 1;  // the last frequency whose first slot is <= slot
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (fr[mid].toff <= *slot) lo = mid;
    else hi = mid - 1;
  }
  *F = fr[lo];
  return true;
}

}  // namespace

__global__ __launch_bounds__(256) void lpsd_window_kernel(const LpsdFreq* __restrict__ fr, double pa, double inv_i0,
                                                          const double* __restrict__ rk2, int64_t woff0,
                                                          double* __restrict__ win) {
  const LpsdFreq F = fr[blockIdx.y];
  double* w = win + (F.woff - woff0);
  for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < F.L; n += (int64_t)gridDim.x * 256)
    w[n] = lpsd_window(n, F.L, pa, inv_i0, rk2);
}

// wsum[2p] = sum w, wsum[2p + 1] = sum w^2 of frequency p of the batch
__global__ __launch_bounds__(256) void lpsd_wsum_kernel(const LpsdFreq* __restrict__ fr, int64_t woff0,
                                                        const double* __restrict__ win, double* __restrict__ wsum) {
  __shared__ double lds[4];
  const LpsdFreq F = fr[blockIdx.x];
  const double* w = win + (F.woff - woff0);
  double s1 = 0.0, s2 = 0.0;
  for (int64_t n = threadIdx.x; n < F.L; n += 256) {
    const double v = w[n];
    s1 += v;
    s2 = fma(v, v, s2);
  }
  s1 = block_sum(s1, lds);
  s2 = block_sum(s2, lds);
  if (threadIdx.x == 0) {
    wsum[2 * blockIdx.x] = s1;
    wsum[2 * blockIdx.x + 1] = s2;
  }
}

// fr: the nf frequencies of this launch (one class of one batch), their tile slots
// [fr[0].toff, fr[0].toff + ntiles) in order. blockIdx.y = series.
//   tile[ser * tiles_ld + (slot - toff0)] = |A|^2
template <int TEAM>
__global__ __launch_bounds__(256) void lpsd_tile_kernel(const double* __restrict__ x, int64_t ser_stride, int64_t N,
                                                        const LpsdFreq* __restrict__ fr, int nf, int64_t ntiles,
                                                        int order, int64_t woff0, const double* __restrict__ win,
                                                        int64_t toff0, int64_t tiles_ld, double* __restrict__ tile) {
  __shared__ double lds[4];
  constexpr int kTilesPerBlock = 256 / TEAM;
  const int lane = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  const int64_t t = (int64_t)blockIdx.x * kTilesPerBlock + (TEAM == 64 ? (int)(threadIdx.x >> 6) : 0);
  if (t >= ntiles) return;  // a whole team leaves together (TEAM = 256: the whole workgroup)
  const int64_t slot = fr[0].toff + t;
  int lo = 0, hi = nf - 1;  // the last frequency whose first slot is <= slot
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (fr[mid].toff <= slot) lo = mid;
    else hi = mid - 1;
  }
  const LpsdFreq F = fr[lo];
  const int64_t s = lpsd_start(slot - F.toff, F.K, F.L, N);
  const double* xs = x + (int64_t)blockIdx.y * ser_stride + s;
  const double* w = win + (F.woff - woff0);
  double mean = 0.0;
  if (order == 0) mean = team_sum<TEAM>(lpsd_share_sum(xs, F.L, lane, TEAM), lds) / (double)F.L;
  double re, im;
  lpsd_share_bin(xs, w, F.L, F.b, mean, lane, TEAM, &re, &im);
  re = team_sum<TEAM>(re, lds);
  im = team_sum<TEAM>(im, lds);
  if (lane == 0) tile[(int64_t)blockIdx.y * tiles_ld + (slot - toff0)] = re * re + im * im;
}

// grid (frequency of the batch, series): Sxx[ser * J + j] = 2 mean_k |A|^2 / (fs sum w^2);
// series 0 also writes enbw[j] = fs sum w^2 / (sum w)^2.
__global__ __launch_bounds__(256) void lpsd_finish_kernel(const LpsdFreq* __restrict__ fr, double fs, int64_t toff0,
                                                          int64_t tiles_ld, const double* __restrict__ tile,
                                                          const double* __restrict__ wsum, int64_t J,
                                                          double* __restrict__ Sxx, double* __restrict__ enbw) {
  __shared__ double lds[4];
  const LpsdFreq F = fr[blockIdx.x];
  const double* p = tile + (int64_t)blockIdx.y * tiles_ld + (F.toff - toff0);
  double a = 0.0;
  for (int64_t k = threadIdx.x; k < F.K; k += 256) a += p[k];
  a = block_sum(a, lds);
  if (threadIdx.x == 0) {
    const double s1 = wsum[2 * blockIdx.x], s2 = wsum[2 * blockIdx.x + 1];
    Sxx[(int64_t)blockIdx.y * J + F.j] = 2.0 * (a / (double)F.K) / (fs * s2);
    if (blockIdx.y == 0) enbw[F.j] = fs * s2 / (s1 * s1);
  }
}

// The pair form of lpsd_tile_kernel (dfmi_lcsd): blockIdx.y = pair (x_stride 0: one x for every
// y). Both means, then A and B with one phasor per sample; the same reductions in the same
// order, so |A|^2 and |B|^2 are lpsd_tile_kernel's bits. Four planes per pair, plane-major:
//   tile[(pair * 4 + q) * tiles_ld + (slot - toff0)] = |A|^2, |B|^2, Re conj(A) B, Im conj(A) B
template <int TEAM>
__global__ __launch_bounds__(256) void lcsd_tile_kernel(const double* __restrict__ x, int64_t x_stride,
                                                        const double* __restrict__ y, int64_t y_stride, int64_t N,
                                                        const LpsdFreq* __restrict__ fr, int nf, int64_t ntiles,
                                                        int order, int64_t woff0, const double* __restrict__ win,
                                                        int64_t toff0, int64_t tiles_ld, double* __restrict__ tile) {
  __shared__ double lds[4];
  const int lane = TEAM == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
  LpsdFreq F;
  int64_t slot;
  if (!team_tile<TEAM>(fr, nf, ntiles, &F, &slot)) return;
  const int64_t s = lpsd_start(slot - F.toff, F.K, F.L, N);
  const double* xs = x + (int64_t)blockIdx.y * x_stride + s;
  const double* ys = y + (int64_t)blockIdx.y * y_stride + s;
  const double* w = win + (F.woff - woff0);
  double mx = 0.0, my = 0.0;
  if (order == 0) {
    mx = team_sum<TEAM>(lpsd_share_sum(xs, F.L, lane, TEAM), lds) / (double)F.L;
    my = team_sum<TEAM>(lpsd_share_sum(ys, F.L, lane, TEAM), lds) / (double)F.L;
  }
  double ar, ai, br, bi;
  lpsd_share_bin2(xs, ys, w, F.L, F.b, mx, my, lane, TEAM, &ar, &ai, &br, &bi);
  ar = team_sum<TEAM>(ar, lds);
  ai = team_sum<TEAM>(ai, lds);
  br = team_sum<TEAM>(br, lds);
  bi = team_sum<TEAM>(bi, lds);
  if (lane == 0) {
    double* p = tile + (int64_t)blockIdx.y * 4 * tiles_ld + (slot - toff0);
    p[0] = ar * ar + ai * ai;
    p[tiles_ld] = br * br + bi * bi;
    p[2 * tiles_ld] = ar * br + ai * bi;
    p[3 * tiles_ld] = ar * bi - ai * br;
  }
}

// grid (frequency of the batch, pair): each plane's K values summed in lpsd_finish_kernel's
// order; out[pair * J + j] for every output that is not NULL, enbw[j] from pair 0.
//   coh = |Sxy|^2 / (Sxx Syy), not clamped; NaN where Sxx Syy = 0
__global__ __launch_bounds__(256) void lcsd_finish_kernel(const LpsdFreq* __restrict__ fr, double fs, int64_t toff0,
                                                          int64_t tiles_ld, const double* __restrict__ tile,
                                                          const double* __restrict__ wsum, int64_t J,
                                                          double* __restrict__ Sxx, double* __restrict__ Syy,
                                                          double* __restrict__ Sxy_re, double* __restrict__ Sxy_im,
                                                          double* __restrict__ coh, double* __restrict__ enbw) {
  __shared__ double lds[4];
  const LpsdFreq F = fr[blockIdx.x];
  const double* p = tile + (int64_t)blockIdx.y * 4 * tiles_ld + (F.toff - toff0);
  double a[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = 0.0;
    for (int64_t k = threadIdx.x; k < F.K; k += 256) v += p[q * tiles_ld + k];
    a[q] = block_sum(v, lds);
  }
  if (threadIdx.x == 0) {
    const double s1 = wsum[2 * blockIdx.x], s2 = wsum[2 * blockIdx.x + 1];
    const double sxx = 2.0 * (a[0] / (double)F.K) / (fs * s2);
    const double syy = 2.0 * (a[1] / (double)F.K) / (fs * s2);
    const double re = 2.0 * (a[2] / (double)F.K) / (fs * s2);
    const double im = 2.0 * (a[3] / (double)F.K) / (fs * s2);
    const int64_t o = (int64_t)blockIdx.y * J + F.j;
    if (Sxx) Sxx[o] = sxx;
    if (Syy) Syy[o] = syy;
    if (Sxy_re) Sxy_re[o] = re;
    if (Sxy_im) Sxy_im[o] = im;
    if (coh) coh[o] = lcsd_coherence(sxx, syy, re, im);
    if (enbw && blockIdx.y == 0) enbw[F.j] = fs * s2 / (s1 * s1);
  }
}

namespace {

// The window rows of a batch's nf frequencies and their sums.
void window_launch(const LpsdFreq* fr, int nf, int64_t maxL, double pa, double inv_i0, const double* rk2, int64_t woff0,
                   double* win, double* wsum, hipStream_t st) {
  int64_t gx = (maxL + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(lpsd_window_kernel, dim3((unsigned)gx, (unsigned)nf), dim3(256), 0, st, fr, pa, inv_i0, rk2, woff0,
                     win);
  hipLaunchKernelGGL(lpsd_wsum_kernel, dim3((unsigned)nf), dim3(256), 0, st, fr, woff0, win, wsum);
}

}  // namespace

// One batch: frequencies fr[0 .. nf) (device table, sorted longest first; the first n256 of
// them have L > kLpsdWaveL), their window rows from woff0 and tile slots from toff0.
hipError_t lpsd_batch_launch(const double* x, int64_t nser, int64_t ser_stride, int64_t N, double fs,
                             const LpsdFreq* fr, int nf, int n256, int64_t maxL, int64_t tiles256, int64_t tiles64,
                             int order, double pa, double inv_i0, const double* rk2, int64_t woff0, double* win,
                             double* wsum, int64_t toff0, int64_t tiles_ld, double* tile, int64_t J, double* Sxx,
                             double* enbw, hipStream_t st) {
  if (nf <= 0) return hipSuccess;
  window_launch(fr, nf, maxL, pa, inv_i0, rk2, woff0, win, wsum, st);
  if (tiles256 > 0)
    hipLaunchKernelGGL(lpsd_tile_kernel<256>, dim3((unsigned)tiles256, (unsigned)nser), dim3(256), 0, st, x, ser_stride,
                       N, fr, n256, tiles256, order, woff0, win, toff0, tiles_ld, tile);
  if (tiles64 > 0)
    hipLaunchKernelGGL(lpsd_tile_kernel<64>, dim3((unsigned)((tiles64 + 3) / 4), (unsigned)nser), dim3(256), 0, st, x,
                       ser_stride, N, fr + n256, nf - n256, tiles64, order, woff0, win, toff0, tiles_ld, tile);
  hipLaunchKernelGGL(lpsd_finish_kernel, dim3((unsigned)nf, (unsigned)nser), dim3(256), 0, st, fr, fs, toff0, tiles_ld,
                     tile, wsum, J, Sxx, enbw);
  return hipGetLastError();
}

// The same batch for dfmi_lcsd: npair pairs (x + p x_stride, y + p y_stride); tile holds
// 4 npair planes of tiles_ld slots.
hipError_t lcsd_batch_launch(const double* x, int64_t x_stride, const double* y, int64_t y_stride, int64_t npair,
                             int64_t N, double fs, const LpsdFreq* fr, int nf, int n256, int64_t maxL, int64_t tiles256,
                             int64_t tiles64, int order, double pa, double inv_i0, const double* rk2, int64_t woff0,
                             double* win, double* wsum, int64_t toff0, int64_t tiles_ld, double* tile, int64_t J,
                             double* Sxx, double* Syy, double* Sxy_re, double* Sxy_im, double* coh, double* enbw,
                             hipStream_t st) {
  if (nf <= 0) return hipSuccess;
  window_launch(fr, nf, maxL, pa, inv_i0, rk2, woff0, win, wsum, st);
  if (tiles256 > 0)
    hipLaunchKernelGGL(lcsd_tile_kernel<256>, dim3((unsigned)tiles256, (unsigned)npair), dim3(256), 0, st, x, x_stride, y,
                       y_stride, N, fr, n256, tiles256, order, woff0, win, toff0, tiles_ld, tile);
  if (tiles64 > 0)
    hipLaunchKernelGGL(lcsd_tile_kernel<64>, dim3((unsigned)((tiles64 + 3) / 4), (unsigned)npair), dim3(256), 0, st, x,
                       x_stride, y, y_stride, N, fr + n256, nf - n256, tiles64, order, woff0, win, toff0, tiles_ld, tile);
  hipLaunchKernelGGL(lcsd_finish_kernel, dim3((unsigned)nf, (unsigned)npair), dim3(256), 0, st, fr, fs, toff0, tiles_ld,
                     tile, wsum, J, Sxx, Syy, Sxy_re, Sxy_im, coh, enbw);
  return hipGetLastError();
}

}  // namespace dfmi
