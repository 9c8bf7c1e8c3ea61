// Rolling forecasts beyond the model's horizon (DESIGN.md §7 "Rolling forecasts", prediff_amd/rollout.py): the pass between two
// sampler runs.  Channels-last fp32, no 16-bit operands (one build, no pd_call_opts).
//   pd_context_advance: with cat = [ctx ; z_scale * z] along T (T_in + T_out frames), ctx_next = cat[stride : stride + T_in], window by
//   window, and forecast[:, f_off : f_off + f_cnt] = z[:, : f_cnt], unscaled.
// ctx / ctx_next are window stacks (B, nwin, T_in, h, w, C) and z is the canvas (B, T_out, Hc, Wc, C) the windows are cut from; the
// plain module is nwin = 1, (h, w) = (Hc, Wc), origin (0, 0).  One HBM-bound launch for both outputs: the folded index runs over the
// elements of ctx_next first and over the f_cnt forecast frames after them, one thread per OUTPUT element (a float4 of channels when
// C % 4 == 0 and every buffer is 16-byte aligned, else one float), 256 threads, grid-stride loop, 64-bit element offsets.  Every output
// element is written exactly once, nothing else is touched; there are no atomics and nothing is read back, so the launch can be captured.
// The scaled branch is ONE fp32 multiply per element (z_scale = float32(1 / scale_factor), rounded by the caller); the other two are copies.
#include "chan_vec.h"

__device__ __forceinline__ float vscale(float s, float v) { return s * v; }
__device__ __forceinline__ float4 vscale(float s, const float4& v) { return make_float4(s * v.x, s * v.y, s * v.z, s * v.w); }

// Cv = C / V channel groups per cell; n_ctx = B nwin T_in h w Cv, total = n_ctx + B f_cnt Hc Wc Cv.  1 <= stride <= T_out, so the frame
// i + stride - T_in read from z lies in [0, T_out).  A window whose origin lies outside [0, Hc - h] x [0, Wc - w] reads nothing from z
// and its new frames are written as zeros (as pd_window_gather).
template <int V>
__global__ void __launch_bounds__(256) context_advance_kernel(const float* __restrict__ ctx, const float* __restrict__ z,
                                                              const int32_t* __restrict__ origin, float* __restrict__ ctx_next,
                                                              float* __restrict__ forecast, int nwin, int T_in, int T_out, int Hc, int Wc,
                                                              int h, int w, int Cv, int stride, float z_scale, int f_T, int f_off, int f_cnt,
                                                              int64_t n_ctx, int64_t total) {
  typedef typename vec_of<V>::type vec;
  const vec* __restrict__ csrc = (const vec*)ctx;
  const vec* __restrict__ zsrc = (const vec*)z;
  vec* __restrict__ cdst = (vec*)ctx_next;
  vec* __restrict__ fdst = (vec*)forecast;
  const int64_t frame = (int64_t)Hc * Wc * Cv;          // one canvas frame
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (i < n_ctx) {
      const int c = (int)(i % Cv);
      int64_t r = i / Cv;
      const int x = (int)(r % w);
      r /= w;
      const int y = (int)(r % h);
      r /= h;
      const int t = (int)(r % T_in);
      r /= T_in;
      const int k = (int)(r % nwin);
      const int64_t b = r / nwin;
      const int ts = t + stride;
      vec v;
      if (ts < T_in) {
        v = csrc[i + (int64_t)stride * h * w * Cv];      // the same window, `stride` frames later
      } else {
        const int oy = origin[2 * k], ox = origin[2 * k + 1];
        vzero(v);
        if (oy >= 0 && oy <= Hc - h && ox >= 0 && ox <= Wc - w)
          v = vscale(z_scale, zsrc[(((b * T_out + (ts - T_in)) * Hc + (oy + y)) * Wc + (ox + x)) * Cv + c]);
      }
      cdst[i] = v;
    } else {
      const int64_t j = i - n_ctx;                       // over (B, f_cnt, Hc, Wc, Cv)
      const int64_t per = (int64_t)f_cnt * frame;
      const int64_t b = j / per, r = j % per;            // r: offset inside the first f_cnt frames of sample b
      fdst[(b * f_T + f_off) * frame + r] = zsrc[b * T_out * frame + r];
    }
  }
}

extern "C" int pd_context_advance(const float* ctx, const float* z, const int32_t* origin_yx, float* ctx_next, float* forecast, int B,
                                  int nwin, int T_in, int T_out, int Hc, int Wc, int h, int w, int C, int stride, float z_scale, int f_T,
                                  int f_off, int f_cnt, pd_stream_t stream) {
  PD_CHECK_ARG(ctx && z && origin_yx && ctx_next && B > 0 && nwin > 0 && T_in > 0 && T_out > 0 && C > 0 && h > 0 && w > 0 && Hc >= h && Wc >= w,
               "pd_context_advance: bad args (B=%d nwin=%d T_in=%d T_out=%d canvas %d x %d, window %d x %d, C=%d)", B, nwin, T_in, T_out, Hc,
               Wc, h, w, C);
  PD_CHECK_ARG(stride >= 1 && stride <= T_out, "pd_context_advance: stride %d outside [1, T_out = %d]", stride, T_out);
  PD_CHECK_ARG(f_cnt >= 0 && f_cnt <= T_out && (f_cnt == 0 || (forecast && f_off >= 0 && f_T > 0 && f_off <= f_T - f_cnt)),
               "pd_context_advance: forecast frames [%d, %d + %d) do not fit f_T = %d / T_out = %d (or forecast is null)", f_off, f_off,
               f_cnt, f_T, T_out);
  PD_CHECK_ARG(ctx_next != ctx && ctx_next != z && (f_cnt == 0 || (forecast != z && forecast != ctx && forecast != ctx_next)),
               "pd_context_advance: an output aliases an input");
  const bool v4 = C % 4 == 0 && aligned16(ctx) && aligned16(z) && aligned16(ctx_next) && (f_cnt == 0 || aligned16(forecast));
  const int Cv = v4 ? C / 4 : C;
  const int64_t n_ctx = (int64_t)B * nwin * T_in * h * w * Cv;
  const int64_t total = n_ctx + (int64_t)B * f_cnt * Hc * Wc * Cv;
  if (v4)
    hipLaunchKernelGGL(context_advance_kernel<4>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, ctx, z, origin_yx, ctx_next, forecast,
                       nwin, T_in, T_out, Hc, Wc, h, w, Cv, stride, z_scale, f_T, f_off, f_cnt, n_ctx, total);
  else
    hipLaunchKernelGGL(context_advance_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, ctx, z, origin_yx, ctx_next, forecast,
                       nwin, T_in, T_out, Hc, Wc, h, w, Cv, stride, z_scale, f_T, f_off, f_cnt, n_ctx, total);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
