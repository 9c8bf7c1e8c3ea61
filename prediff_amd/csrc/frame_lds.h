// What the kernels that keep one whole frame in LDS share (steps.hip, anvil.hip): the frame limits of the LDS-resident transform, the
// fixed-order fp64 workgroup sum, pd_advect's bilinear rule with fill 0, the pixel loop of a 1024-thread workgroup and the 2-D transform
// of the padded complex frame (pitch W + 1) around the FFT core of fft_lds.h.  Moved here from steps.hip as they stood.
#pragma once
#include <algorithm>
#include "common.h"
#include "fft_lds.h"

namespace {

constexpr int ST_THREADS = 1024;
constexpr int ST_MIN_SIDE = 8, ST_MAX_SIDE = 512, ST_MAX_ELEMS = ST_THREADS * SP_PER_THREAD, ST_MAX_LEVELS = 8;
constexpr int ST_MAX_LEADS = 4096, ST_MAX_BATCH = 65535;
constexpr int ST_RED = 4 * 16;                                 // doubles of block_sum's LDS: up to 4 sums of 16 waves
constexpr int ST_LDS_LIMIT = 160 * 1024 - 512;
constexpr float ST_FAR = 1048576.f;                            // 2^20, pd_advect's

__device__ __forceinline__ double st_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v[n] <- the sum of v[n] over the workgroup, the same bits in every thread.  red: ST_RED doubles of LDS.
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* __restrict__ red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = st_wave_sum(v[n]);
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

// pd_advect's rule with fill 0: bilinear from floor, a tap outside the frame reads 0; a coordinate that is not finite or further than 2^20
// from the frame gives 0 before any integer is made of it
__device__ __forceinline__ float st_bil_fill(const float* __restrict__ I, int H, int W, float cy, float cx) {
  float r = 0.f;
  if (cy >= -ST_FAR && cy <= (float)(H - 1) + ST_FAR && cx >= -ST_FAR && cx <= (float)(W - 1) + ST_FAR) {
    const float y0f = floorf(cy), x0f = floorf(cx);
    const float fy = cy - y0f, fx = cx - x0f;
    const int y0 = (int)y0f, x0 = (int)x0f;
    const bool r0 = y0 >= 0 && y0 < H, r1 = y0 + 1 >= 0 && y0 + 1 < H;
    const bool c0 = x0 >= 0 && x0 < W, c1 = x0 + 1 >= 0 && x0 + 1 < W;
    const float i00 = r0 && c0 ? I[y0 * W + x0] : 0.f;
    const float i01 = r0 && c1 ? I[y0 * W + x0 + 1] : 0.f;
    const float i10 = r1 && c0 ? I[(y0 + 1) * W + x0] : 0.f;
    const float i11 = r1 && c1 ? I[(y0 + 1) * W + x0 + 1] : 0.f;
    const float top = i00 + fx * (i01 - i00);
    const float bot = i10 + fx * (i11 - i10);
    r = top + fy * (bot - top);
  }
  return r;
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

bool st_side_ok(int64_t n) {
  if (n < ST_MIN_SIDE || n > ST_MAX_SIDE) return false;
  if (n % 3 == 0) n /= 3;
  return (n & (n - 1)) == 0;
}

bool st_frame_ok(int H, int W) { return st_side_ok(H) && st_side_ok(W) && (int64_t)H * W <= ST_MAX_ELEMS; }

bool st_levels_ok(int H, int W, int levels) {
  int lg = 0;
  for (int m = std::max(H, W); m > 1; m >>= 1) ++lg;             // floor(log2(max(H, W)))
  return levels >= 2 && levels <= lg - 1 && levels <= ST_MAX_LEVELS;
}

int st_raise_lds(const char* who, const void* fn, bool* done) {
  bool& set = done[pd_cur_device()];
  if (!set) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_LIMIT);
    if (e != hipSuccess) {
      pd_set_error("%s: hipFuncSetAttribute(%d) failed: %s", who, ST_LDS_LIMIT, hipGetErrorString(e));
      return PD_ERR_LAUNCH;
    }
    set = true;
  }
  return PD_OK;
}

size_t st_frame_lds(int H, int W) { return sizeof(float2) * ((size_t)H * (W + 1) + std::max(H, W)) + sizeof(double) * ST_RED; }

}  // namespace
