// The SEVIR pixel front end (DESIGN.md §7 "SEVIR pixel front end", prediff_amd/sevir_io.py): raw VIL events in, model frames out, and
// back.  No 16-bit operands (one build, no pd_call_opts).
//   pd_sevir_ingest: uint8 raw (N, H, W, T) -> fp32 (N * nwin, in_len | out_len, H / fh, W / fw, 1): every ft-th frame, the maximum of the
//   bytes of each fh x fw block (save_downsampled_dataset, sevir_dataloader.py:460-467), then scale * (float(x) + offset) as ONE fp32 add
//   and ONE fp32 multiply (preprocess_data_dict, :645).  One launch, no intermediate tensor.
//   pd_sevir_export: fp32 (B, T, H, W, 1) -> x / scale - offset, ONE fp32 divide (correctly rounded) and ONE fp32 subtract
//   (process_data_dict_back, :679), written as fp32 or clamped to [0, 255], rounded half to even and written as bytes (NTHW or NHWT).
// The arithmetic is written so that no operation pair can contract into an fma (fp contract off in the two value functions), and the
// library is built without fast-math: `/` is the IEEE division (v_div_scale / v_div_fmas / v_div_fixup).
//
// Ingest, the memory side.  T is the innermost raw axis, so the bytes behind `cols` LR cells of one LR row h' are fh contiguous segments
// of cols fw T bytes, one per raw row (v1: rows of 384 * 49 = 18 816 bytes), of which the strided frames and the block maximum use a
// scattered subset.  A workgroup owns (n, h', a chunk of Wc LR columns): it copies its fh segments into LDS with 16-byte loads (whole
// 16-byte granules of the ADDRESS: a segment starts anywhere, T is odd, so up to 15 head and 15 tail bytes go byte by byte, and nothing
// outside the segment is read), keeping each byte at its global offset inside its granule so that a 16-byte global load is a 16-byte
// LDS write; after one barrier a thread per (window, frame, x') takes the block maximum from LDS and writes its float, x' fastest:
// contiguous fp32 row pieces.  Wc is the largest even split of the row whose segments fit SEVIR_LDS_BUDGET.  The budget is small on
// purpose: a workgroup is a load phase, a barrier and a store phase, and only other resident workgroups overlap them -- staging the
// whole v1 run (56 448 bytes, two workgroups per CU) ran at 2.80 TB/s, 32 KiB at 3.32, 20 KiB (three chunks, eight workgroups per CU)
// at 3.50, the rate of a plain device copy in the same run (profiles/time_sevir_io.log has the last).
#include "common.h"

#define SEVIR_THREADS 256
#define SEVIR_LDS_BUDGET 20480

__device__ __forceinline__ float sevir_forward(unsigned byte, float scale, float offset) {
#pragma clang fp contract(off)
  const float s = (float)byte + offset;
  return scale * s;
}
__device__ __forceinline__ float sevir_back(float x, float scale, float offset) {
#pragma clang fp contract(off)
  const float q = x / scale;
  return q - offset;
}
// [0, 255], half to even (torch.round); a NaN becomes 0 (fmaxf returns the other operand)
__device__ __forceinline__ unsigned sevir_byte(float v) { return (unsigned)rintf(fminf(fmaxf(v, 0.f), 255.f)); }

// grid: nchunk * Hl * N workgroups, chunk fastest.  Segment r (raw row h' fh + r, cols * fw * T bytes) sits at LDS offset r * seg_pitch;
// seg_pitch >= 15 + the longest segment, a multiple of 16.
__global__ void __launch_bounds__(SEVIR_THREADS) sevir_ingest_kernel(const uint8_t* __restrict__ raw, const int32_t* __restrict__ starts,
                                                                     float* __restrict__ ctx, float* __restrict__ tgt, int H, int W, int T,
                                                                     int ft, int fh, int fw, int Hl, int Wl, int T_lr, int Wc, int nchunk,
                                                                     int seg_pitch, int nwin, int in_len, int out_len,
                                                                     float scale, float offset) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sevir_lds[];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.x % nchunk;
  const int hl = (blockIdx.x / nchunk) % Hl;
  const int n = blockIdx.x / nchunk / Hl;
  const int w0 = chunk * Wc, cols = min(Wc, Wl - w0);
  const int WT = W * T;                                                   // one raw row (the host checks it against int)
  const uint8_t* __restrict__ g0 = raw + (((int64_t)n * H + (int64_t)hl * fh) * W + (int64_t)w0 * fw) * T;
  const int seg_len = cols * fw * T;

  for (int s = 0; s < fh; ++s) {
    const uint8_t* __restrict__ g = g0 + (int64_t)s * WT;
    const int ph = (int)((uintptr_t)g & 15);                              // byte i of the segment lives at l[ph + i]
    uint8_t* l = sevir_lds + s * seg_pitch;
    const int head = min(seg_len, (16 - ph) & 15);
    const int nvec = (seg_len - head) >> 4;
    const int tail0 = head + (nvec << 4);
    if (nvec > 0) {
      const uint4* __restrict__ gv = (const uint4*)(g + head);            // 16-byte aligned: ph + head is a multiple of 16
      uint4* lv = (uint4*)(l + ph + head);
#pragma unroll 4
      for (int i = tid; i < nvec; i += SEVIR_THREADS) lv[i] = gv[i];
    }
    if (tid < head) l[ph + tid] = g[tid];
    const int tt = tid - 16;                                              // threads 16 .. 31: the tail (< 16 bytes)
    if (tt >= 0 && tail0 + tt < seg_len) l[ph + tail0 + tt] = g[tail0 + tt];
  }
  __syncthreads();

  const int ph0 = (int)((uintptr_t)g0 & 15);
  const int nf = in_len + out_len;
  const int items = nwin * nf * cols;
  for (int i = tid; i < items; i += SEVIR_THREADS) {
    const int x = i % cols, q = i / cols;
    const int j = q % nf, k = q / nf;
    const int st = starts[k];
    float v = 0.f;
    if (st >= 0 && st <= T_lr - nf) {                                     // a window outside the event reads nothing and is written as zeros
      const int col = (x * fw) * T + (st + j) * ft;
      unsigned m = 0;
      for (int r = 0; r < fh; ++r) {
        const uint8_t* row = sevir_lds + r * seg_pitch + ((ph0 + r * (WT & 15)) & 15) + col;
        for (int c = 0; c < fw; ++c) m = max(m, (unsigned)row[c * T]);
      }
      v = sevir_forward(m, scale, offset);
    }
    const int64_t seq = (int64_t)n * nwin + k;
    if (j < in_len)
      ctx[((seq * in_len + j) * Hl + hl) * Wl + w0 + x] = v;
    else
      tgt[((seq * out_len + (j - in_len)) * Hl + hl) * Wl + w0 + x] = v;
  }
}

extern "C" int pd_sevir_ingest(const uint8_t* raw, const int32_t* starts, float* ctx, float* tgt, int N, int H, int W, int T, int ft, int fh,
                               int fw, int nwin, int in_len, int out_len, float scale, float offset, pd_stream_t stream) {
  PD_CHECK_ARG(raw && starts && ctx && N > 0 && H > 0 && W > 0 && T > 0 && ft > 0 && fh > 0 && fw > 0 && nwin > 0 && in_len > 0 && out_len >= 0,
               "pd_sevir_ingest: bad args (raw (%d, %d, %d, %d), factors (%d, %d, %d), nwin=%d in_len=%d out_len=%d)", N, H, W, T, ft, fh, fw,
               nwin, in_len, out_len);
  PD_CHECK_ARG((out_len == 0) == (tgt == nullptr), "pd_sevir_ingest: tgt must be null exactly when out_len = 0 (out_len=%d)", out_len);
  PD_CHECK_ARG(H % fh == 0 && W % fw == 0, "pd_sevir_ingest: %d x %d is not divisible by the factors %d x %d", H, W, fh, fw);
  const int Hl = H / fh, Wl = W / fw, T_lr = (T + ft - 1) / ft, nf = in_len + out_len;
  PD_CHECK_ARG(nf <= T_lr, "pd_sevir_ingest: windows of %d + %d frames on %d LR frames (T=%d, ft=%d)", in_len, out_len, T_lr, T, ft);
  const int64_t row_bytes = (int64_t)W * T, block_bytes = (int64_t)fw * T;
  // one workgroup's (window, frame, x') items and its LDS offsets are ints
  PD_CHECK_ARG((int64_t)nwin * nf * Wl < (1 << 30) && row_bytes < (1 << 30), "pd_sevir_ingest: %d windows of %d frames on rows of %d "
               "cells (%lld raw bytes per row): too large", nwin, nf, Wl, (long long)row_bytes);
  // the most LR columns whose fh segments (each with its alignment slack) fit the budget, then an even split of the row
  const int64_t per_seg = SEVIR_LDS_BUDGET / fh / 16 * 16 - 15;
  PD_CHECK_ARG(per_seg >= block_bytes, "pd_sevir_ingest: one %d x %d block of %d frames does not fit the LDS budget", fh, fw, T);
  const int64_t fit = per_seg / block_bytes;
  int nchunk = (int)((Wl + fit - 1) / fit);
  const int Wc = (Wl + nchunk - 1) / nchunk;
  nchunk = (Wl + Wc - 1) / Wc;
  const int64_t seg_pitch = ((int64_t)Wc * block_bytes + 15 + 15) / 16 * 16;
  const int64_t lds = seg_pitch * fh;
  const int64_t grid = (int64_t)nchunk * Hl * N;
  PD_CHECK_ARG(lds <= SEVIR_LDS_BUDGET && grid <= 0x7fffffff, "pd_sevir_ingest: %lld bytes of LDS / %lld workgroups", (long long)lds, (long long)grid);
  hipLaunchKernelGGL(sevir_ingest_kernel, dim3((unsigned)grid), dim3(SEVIR_THREADS), (size_t)lds, (hipStream_t)stream, raw, starts, ctx, tgt, H,
                     W, T, ft, fh, fw, Hl, Wl, T_lr, Wc, nchunk, (int)seg_pitch, nwin, in_len, out_len, scale, offset);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// One thread per group of four consecutive OUTPUT elements (grid-stride): a float4 / a packed dword when `vec` (both buffers aligned for
// it) and the group is whole, element by element otherwise.  NHWT reads frame t of pixel p = (b, h, w) at ((b T + t) HW + hw).
template <int MODE>
__global__ void __launch_bounds__(256) sevir_export_kernel(const float* __restrict__ x, void* __restrict__ out, int64_t n, int T, int64_t HW,
                                                           float scale, float offset, int vec) {
  const int64_t ngroup = (n + 3) / 4;
  for (int64_t gidx = (int64_t)blockIdx.x * 256 + threadIdx.x; gidx < ngroup; gidx += (int64_t)gridDim.x * 256) {
    const int64_t o = gidx * 4;
    const int cnt = (int)min((int64_t)4, n - o);
    float v[4];
    if (MODE != PD_SEVIR_U8_NHWT && vec && cnt == 4) {
      const float4 q = *(const float4*)(x + o);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int64_t src = min(o + e, n - 1);
        if (MODE == PD_SEVIR_U8_NHWT) {
          const int64_t p = src / T;
          const int t = (int)(src - p * T);
          src = ((p / HW) * T + t) * HW + p % HW;
        }
        v[e] = x[src];
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = sevir_back(v[e], scale, offset);
    if (MODE == PD_SEVIR_F32) {
      float* dst = (float*)out + o;
      if (vec && cnt == 4) {
        *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) dst[e] = v[e];
      }
    } else {
      uint8_t* dst = (uint8_t*)out + o;
      const unsigned b0 = sevir_byte(v[0]), b1 = sevir_byte(v[1]), b2 = sevir_byte(v[2]), b3 = sevir_byte(v[3]);
      if (vec && cnt == 4) {
        *(uint32_t*)dst = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
      } else {
        const unsigned b[4] = {b0, b1, b2, b3};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) dst[e] = (uint8_t)b[e];
      }
    }
  }
}

extern "C" int pd_sevir_export(const float* x, void* out, int64_t B, int T, int H, int W, float scale, float offset, int mode,
                               pd_stream_t stream) {
  PD_CHECK_ARG(x && out && B > 0 && T > 0 && H > 0 && W > 0, "pd_sevir_export: bad args (x (%lld, %d, %d, %d, 1))", (long long)B, T, H, W);
  PD_CHECK_ARG(mode == PD_SEVIR_F32 || mode == PD_SEVIR_U8_NTHW || mode == PD_SEVIR_U8_NHWT, "pd_sevir_export: unknown mode %d", mode);
  PD_CHECK_ARG(scale != 0.f && (const void*)x != out, "pd_sevir_export: scale is 0, or out aliases x");
  const int64_t HW = (int64_t)H * W, n = B * T * HW;
  const int vec = ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & (mode == PD_SEVIR_F32 ? 15 : 3)) == 0;
  const unsigned grid = (unsigned)min((int64_t)8192, ((n + 3) / 4 + 255) / 256);
  if (mode == PD_SEVIR_F32)
    hipLaunchKernelGGL(sevir_export_kernel<PD_SEVIR_F32>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, n, T, HW, scale, offset, vec);
  else if (mode == PD_SEVIR_U8_NTHW)
    hipLaunchKernelGGL(sevir_export_kernel<PD_SEVIR_U8_NTHW>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, n, T, HW, scale, offset, vec);
  else
    hipLaunchKernelGGL(sevir_export_kernel<PD_SEVIR_U8_NHWT>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, n, T, HW, scale, offset, vec);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
