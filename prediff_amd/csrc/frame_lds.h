// What the kernels that keep one whole frame in LDS share (steps.hip, anvil.hip): the frame limits of the LDS-resident transform, the
// fixed-order fp64 workgroup sum, the pixel loop of a 1024-thread workgroup and the 2-D transform of the padded complex frame
// (pitch W + 1) around the FFT core of fft_lds.h.  What they share with other files is included, not restated: the side rule and
// its limits (fft_lds.h, with spectrum.hip), pd_advect's bilinear rule (bilinear.h, with extrapolation.hip), the fp64 wave sum and the
// dynamic-LDS raise (common.h).
#pragma once
#include <algorithm>
#include "bilinear.h"
#include "common.h"
#include "fft_lds.h"

namespace {

constexpr int ST_THREADS = 1024;
constexpr int ST_MAX_ELEMS = ST_THREADS * SP_PER_THREAD, ST_MAX_LEVELS = 8;
constexpr int ST_MAX_LEADS = 4096, ST_MAX_BATCH = 65535;
constexpr int ST_RED = 4 * 16;                                 // doubles of block_sum's LDS: up to 4 sums of 16 waves
constexpr int ST_LDS_LIMIT = 160 * 1024 - 512;

// v[n] <- the sum of v[n] over the workgroup, the same bits in every thread.  red: ST_RED doubles of LDS.
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* __restrict__ red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = wave_sum_f64(v[n]);
  __syncthreads();                                             // the last reader of red is done
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[n * 16 + wave] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    double a = 0.0;
    for (int w = 0; w < nw; ++w) a += red[n * 16 + w];
    v[n] = a;
  }
}

// the pixels of a thread: i = threadIdx.x + j ST_THREADS, j < SP_PER_THREAD; ST_PIXELS(body) runs body with i, y, x, li (the LDS index)
#define ST_PIXELS(...)                                                     \
  _Pragma("unroll 1") for (int j = 0; j < SP_PER_THREAD; ++j) {            \
    const int i = (int)threadIdx.x + j * ST_THREADS;                       \
    if (i < HW) {                                                          \
      const int y = i / W, x = i - y * W, li = y * pitch + x;              \
      __VA_ARGS__                                                          \
    }                                                                      \
  }

__device__ __forceinline__ void fft2d(float2* __restrict__ z, float2* __restrict__ tw, int H, int W, int pitch) {
  // An empty statement the optimiser cannot see through: without it the stages' per-thread index arithmetic, which depends on H and W
  // only, is hoisted out of the callers' loop of passes, stays live through all of it and spills (137 VGPRs of scratch).
  asm volatile("" : "+s"(H), "+s"(W), "+s"(pitch));
  fft_lines<false>(z, tw, H, W, pitch);
  fft_lines<true>(z, tw, W, H, pitch);
}

bool st_frame_ok(int H, int W) { return sp_side_ok(H) && sp_side_ok(W) && (int64_t)H * W <= ST_MAX_ELEMS; }

bool st_levels_ok(int H, int W, int levels) {
  int lg = 0;
  for (int m = std::max(H, W); m > 1; m >>= 1) ++lg;             // floor(log2(max(H, W)))
  return levels >= 2 && levels <= lg - 1 && levels <= ST_MAX_LEVELS;
}

size_t st_frame_lds(int H, int W) { return sizeof(float2) * ((size_t)H * (W + 1) + std::max(H, W)) + sizeof(double) * ST_RED; }

}  // namespace
