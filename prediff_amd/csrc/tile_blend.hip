// Tiled sampling on a canvas larger than the model's window (prediff_amd/tiled.py): the two passes around the
// denoiser / the VAE decoder.  Channels-last fp32, no 16-bit operands (one build, no pd_call_opts).
//   pd_window_gather: canvas (B, T, Hc, Wc, C) -> windows (B, nwin, T, h, w, C), window k = the h x w patch at origin_yx[k]
//   pd_window_blend : windows -> canvas, canvas(cell) = sum over the windows covering the cell of weight_k(cell) * window_k(cell)
// Both are single HBM-bound passes: one thread per OUTPUT element (a float4 of channels when C % 4 == 0 and the buffers are 16-byte
// aligned, else one float; with C = 1 consecutive threads run along x), 256 threads, grid-stride loop over the folded index.
// The blend is a gather-form reduction: the thread that owns a canvas element walks the windows in ascending index, tests coverage
// and accumulates fmaf(weight, value, acc) from acc = 0 -- no atomics, a fixed summation order, so two launches give the same bits.
// The weights arrive normalised (they sum to 1 over the windows covering a cell; fp64 on the host, rounded once): nothing is divided here.
#include "chan_vec.h"

__device__ __forceinline__ void vfma(float g, float e, float& acc) { acc = fmaf(g, e, acc); }
__device__ __forceinline__ void vfma(float g, const float4& e, float4& acc) {
  acc.x = fmaf(g, e.x, acc.x);
  acc.y = fmaf(g, e.y, acc.y);
  acc.z = fmaf(g, e.z, acc.z);
  acc.w = fmaf(g, e.w, acc.w);
}

// Cv = C / V channel groups per cell.  A window whose origin lies outside [0, Hc - h] x [0, Wc - w] reads nothing and is written as zeros.
template <int V>
__global__ void __launch_bounds__(256) window_gather_kernel(const float* __restrict__ canvas, float* __restrict__ windows,
                                                            const int32_t* __restrict__ origin, int nwin, int T, int Hc, int Wc, int h, int w,
                                                            int Cv, int64_t total) {
  typedef typename vec_of<V>::type vec;
  const vec* __restrict__ src = (const vec*)canvas;
  vec* __restrict__ dst = (vec*)windows;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % Cv);
    int64_t r = i / Cv;
    const int x = (int)(r % w);
    r /= w;
    const int y = (int)(r % h);
    r /= h;
    const int t = (int)(r % T);
    r /= T;
    const int k = (int)(r % nwin);
    const int64_t b = r / nwin;
    const int oy = origin[2 * k], ox = origin[2 * k + 1];
    vec v;
    vzero(v);
    if (oy >= 0 && oy <= Hc - h && ox >= 0 && ox <= Wc - w) v = src[(((b * T + t) * Hc + (oy + y)) * Wc + (ox + x)) * Cv + c];
    dst[i] = v;
  }
}

template <int V>
__global__ void __launch_bounds__(256) window_blend_kernel(const float* __restrict__ windows, const float* __restrict__ weights,
                                                           const int32_t* __restrict__ origin, float* __restrict__ canvas, int nwin, int T,
                                                           int Hc, int Wc, int h, int w, int Cv, int64_t total) {
  typedef typename vec_of<V>::type vec;
  const vec* __restrict__ src = (const vec*)windows;
  vec* __restrict__ dst = (vec*)canvas;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % Cv);
    int64_t r = i / Cv;
    const int x = (int)(r % Wc);
    r /= Wc;
    const int y = (int)(r % Hc);
    r /= Hc;
    const int t = (int)(r % T);
    const int64_t b = r / T;
    vec acc;
    vzero(acc);
    for (int k = 0; k < nwin; ++k) {
      const int wy = y - origin[2 * k], wx = x - origin[2 * k + 1];
      if (wy < 0 || wy >= h || wx < 0 || wx >= w) continue;      // the window-relative cell is in range whatever the table holds
      const float g = weights[((int64_t)k * h + wy) * w + wx];
      vfma(g, src[((((b * nwin + k) * T + t) * h + wy) * w + wx) * Cv + c], acc);
    }
    dst[i] = acc;
  }
}

#define PD_CHECK_TILE_ARGS(name)                                                                                                   \
  PD_CHECK_ARG(canvas && windows && origin_yx && B > 0 && nwin > 0 && T > 0 && C > 0 && h > 0 && w > 0 && Hc >= h && Wc >= w,      \
               name ": bad args (B=%d nwin=%d T=%d canvas %d x %d, window %d x %d, C=%d)", B, nwin, T, Hc, Wc, h, w, C)

extern "C" int pd_window_gather(const float* canvas, float* windows, const int32_t* origin_yx, int B, int nwin, int T, int Hc, int Wc, int h,
                                int w, int C, pd_stream_t stream) {
  PD_CHECK_TILE_ARGS("pd_window_gather");
  const bool v4 = C % 4 == 0 && aligned16(canvas) && aligned16(windows);
  const int Cv = v4 ? C / 4 : C;
  const int64_t total = (int64_t)B * nwin * T * h * w * Cv;
  if (v4)
    hipLaunchKernelGGL(window_gather_kernel<4>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, canvas, windows, origin_yx, nwin, T, Hc,
                       Wc, h, w, Cv, total);
  else
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, canvas, windows, origin_yx, nwin, T, Hc,
                       Wc, h, w, Cv, total);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_window_blend(const float* windows, const float* weights, const int32_t* origin_yx, float* canvas, int B, int nwin, int T,
                               int Hc, int Wc, int h, int w, int C, pd_stream_t stream) {
  PD_CHECK_TILE_ARGS("pd_window_blend");
  PD_CHECK_ARG(weights, "pd_window_blend: weights is null");
  const bool v4 = C % 4 == 0 && aligned16(canvas) && aligned16(windows);
  const int Cv = v4 ? C / 4 : C;
  const int64_t total = (int64_t)B * T * Hc * Wc * Cv;
  if (v4)
    hipLaunchKernelGGL(window_blend_kernel<4>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, windows, weights, origin_yx, canvas, nwin,
                       T, Hc, Wc, h, w, Cv, total);
  else
    hipLaunchKernelGGL(window_blend_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, windows, weights, origin_yx, canvas, nwin,
                       T, Hc, Wc, h, w, Cv, total);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
