// Normalisation / cast kernels: fp32 residual stream in, GEMM A operands out -- 16-bit (bf16 / fp16, or the bf16 hi/lo pair), unit-scale
// e4m3 or MX e4m3.  All HBM-bound: one pass over the row (LayerNorm) or two passes over the sample (GroupNorm: stats, then
// apply+SiLU+cast).  Every producer writes through the one writer family below; the statistics are shared per summation order.
#include "common.h"
#include "mx_quant.h"

namespace PD_NS {

// -------------------------------------------------------------------------------------------------
// Output kinds and their writers.  `out` / `aux` are the bases of row-major buffers and row + c the element index of the first value
// (row = the row's first element, c = the column: kept apart because a row is often wave-uniform):
//   Op16  out = 16-bit operands (pack_op2 / f2op: the build's operand type); aux = the lo half of the bf16 hi/lo split, or null
//   E4M3  out = bytes, e4m3(y * scale) saturating; aux unused
//   MX    out = payload bytes, aux = E8M0 scale bytes, one per 32 elements (mx_quant.h states the format); the row length is a
//         multiple of 32, so the element belongs to block (row >> 5) + (c >> 5) and the lane with c % 32 == 0 writes the block's byte
// -------------------------------------------------------------------------------------------------
enum class Out { Op16, E4M3, MX };

__device__ __forceinline__ uint2 pack_op4(const float (&y)[4]) { return make_uint2(pack_op2(y[0], y[1]), pack_op2(y[2], y[3])); }

// four consecutive values, one packed store per buffer (MX: the 8 lanes of a block call this together)
template <Out OUT>
__device__ __forceinline__ void write4(void* out, void* aux, int64_t row, int c, const float (&y)[4], float scale) {
  const int64_t i = row + c;
  if constexpr (OUT == Out::Op16) {
    if (aux) {
      uint16_t hi[4], lo[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) f2bf_split(y[k], hi[k], lo[k]);
      *(uint2*)((pd_bf16*)out + i) = make_uint2(hi[0] | ((uint32_t)hi[1] << 16), hi[2] | ((uint32_t)hi[3] << 16));
      *(uint2*)((pd_bf16*)aux + i) = make_uint2(lo[0] | ((uint32_t)lo[1] << 16), lo[2] | ((uint32_t)lo[3] << 16));
    } else {
      *(uint2*)((pd_bf16*)out + i) = pack_op4(y);
    }
  } else if constexpr (OUT == Out::E4M3) {
    *(uint32_t*)((uint8_t*)out + i) = pack_e4m3x4(y, scale);
  } else {
    int sb;
    *(uint32_t*)((uint8_t*)out + i) = mx_quantize4(y, sb);
    if ((c & 31) == 0) ((uint8_t*)aux)[(row >> 5) + (c >> 5)] = (uint8_t)sb;
  }
}
// one value (the scalar kernels: 16-bit outputs only)
__device__ __forceinline__ void write1(pd_bf16* out, pd_bf16* out_lo, int64_t i, float y) {
  if (out_lo) {
    uint16_t hi, lo;
    f2bf_split(y, hi, lo);
    out[i] = hi; out_lo[i] = lo;
  } else {
    out[i] = f2op(y);
  }
}

// -------------------------------------------------------------------------------------------------
// LayerNorm over C (affine), one wave per row, two-pass in registers (exact mean / centered variance).
// cuboid_transformer.py:813 / :197 (nn.LayerNorm eps 1e-5, models/utils.py:192-221)
// -------------------------------------------------------------------------------------------------
constexpr int LN_MAXV = 16;   // up to 64*4*16 = 4096 channels per row

// 1 / sqrt(var + eps): the only LayerNorm arithmetic that depends on the output kind.  The MX payload is compared byte for byte with
// tests/_mx_ref.py, so its rstd is the IEEE quotient of the IEEE square root; the other kinds keep the faster rsqrtf.
template <Out OUT>
__device__ __forceinline__ float ln_rstd(float var_eps) { return OUT == Out::MX ? 1.0f / sqrtf(var_eps) : rsqrtf(var_eps); }

// NV = float4 vectors per lane per row (ceil(C/256)), R = rows handled concurrently by one wave (independent load /
// reduce chains keep R x NV 16 B loads in flight per lane: the kernel is pure HBM streaming; MX runs R = 1).
// OUT / out / aux / scale: see write4.  MX: ld_out % 32 == 0, so the 8 lanes of a block pass every branch below together.
template <bool GATHER, int NV, int R, Out OUT>
__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, void* __restrict__ out,
                                                        void* __restrict__ aux, int64_t rows, int C, int ld_out,
                                                        float eps, float scale,
                                                        // patch-merge gather geometry (GATHER only)
                                                        int T, int H, int W, int Cs, int dt, int dh, int dw, int nearest) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= rows) return;
  float4 v[R][NV];
  float s[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    s[r] = 0.f;
    // source row decode for the patch-merge gather: row = ((b*To + to)*Ho + ho)*Wo + wo
    int64_t gb = 0;
    int to = 0, ho = 0, wo = 0;
    if (GATHER) {
      const int To = (T + dt - 1) / dt, Ho = (H + dh - 1) / dh, Wo = (W + dw - 1) / dw;
      int64_t q = row;
      wo = (int)(q % Wo); q /= Wo;
      ho = (int)(q % Ho); q /= Ho;
      to = (int)(q % To); gb = q / To;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = j * 256 + lane * 4;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C && row < rows) {
        if (GATHER) {
          // element e = ((it*dh + ih)*dw + iw)*Cs + cs   (cuboid_transformer.py:286-292)
          const int sub = c / Cs, cs = c - sub * Cs;
          const int iw = sub % dw, ih = (sub / dw) % dh, it = sub / (dw * dh);
          int tt = to * dt + it, hh = ho * dh + ih, ww = wo * dw + iw;
          if (nearest) {
            // padding_type "nearest" (models/utils.py:228-256): the padded grid is F.interpolate(x, size = padded size), i.e. padded
            // coordinate p reads a source coordinate inside the tensor
            // -- with torch's own arithmetic: min(floor(p * float32(size / padded size)), size - 1), which is not the integer floor
            // (22 padded to 26: position 13 reads 10, not 11)
            const int Tp = ((T + dt - 1) / dt) * dt, Hp = ((H + dh - 1) / dh) * dh, Wp = ((W + dw - 1) / dw) * dw;
            tt = min((int)floorf((float)tt * ((float)T / (float)Tp)), T - 1);
            hh = min((int)floorf((float)hh * ((float)H / (float)Hp)), H - 1);
            ww = min((int)floorf((float)ww * ((float)W / (float)Wp)), W - 1);
          }
          if (tt < T && hh < H && ww < W)
            t = *(const float4*)(x + ((((gb * T + tt) * H + hh) * W + ww) * (int64_t)Cs + cs));
        } else {
          t = *(const float4*)(x + row * (int64_t)C + c);
        }
      }
      v[r][j] = t;
      s[r] += (t.x + t.y) + (t.z + t.w);
    }
  }
  float mean[R], rstd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) mean[r] = wave_sum(s[r]) / (float)C;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = j * 256 + lane * 4;
      if (c < C) {
        const float a = v[r][j].x - mean[r], b = v[r][j].y - mean[r], cc = v[r][j].z - mean[r], d = v[r][j].w - mean[r];
        q += (a * a + b * b) + (cc * cc + d * d);
      }
    }
    s[r] = q;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) rstd[r] = ln_rstd<OUT>(wave_sum(s[r]) / (float)C + eps);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = j * 256 + lane * 4;
    if (c >= ld_out) continue;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), be = g;
    if (c < C) { g = *(const float4*)(gamma + c); be = *(const float4*)(beta + c); }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + r;
      if (row >= rows) continue;
      float y[4] = {0.f, 0.f, 0.f, 0.f};
      if (c < C) {
        y[0] = (v[r][j].x - mean[r]) * rstd[r] * g.x + be.x;
        y[1] = (v[r][j].y - mean[r]) * rstd[r] * g.y + be.y;
        y[2] = (v[r][j].z - mean[r]) * rstd[r] * g.z + be.z;
        y[3] = (v[r][j].w - mean[r]) * rstd[r] * g.w + be.w;
      }
      write4<OUT>(out, aux, row * (int64_t)ld_out, c, y, scale);
    }
  }
}

// One launcher for every LayerNorm entry point.  Rows per wave by vector count; MX keeps one row per wave.
template <bool GATHER, Out OUT>
static void launch_layernorm(const float* x, const float* gamma, const float* beta, void* out, void* aux, int64_t rows, int C, int ld_out,
                             float eps, float scale, hipStream_t s, int T = 0, int H = 0, int W = 0, int Cs = 0, int dt = 1, int dh = 1,
                             int dw = 1, int nearest = 0) {
  const int nv = (C + 255) / 256;
#define PD_LN(NV, RR)                                                                                                              \
  do {                                                                                                                             \
    constexpr int R = OUT == Out::MX ? 1 : (RR);                                                                                   \
    hipLaunchKernelGGL((layernorm_kernel<GATHER, NV, R, OUT>), dim3((unsigned)((rows + 4 * R - 1) / (4 * R))), dim3(256), 0, s, x, gamma, \
                       beta, out, aux, rows, C, ld_out, eps, scale, T, H, W, Cs, dt, dh, dw, nearest);                             \
  } while (0)
  if (nv <= 1) PD_LN(1, 4);
  else if (nv <= 2) PD_LN(2, 2);
  else if (nv <= 4) PD_LN(4, 1);
  else if (nv <= 8) PD_LN(8, 1);
  else PD_LN(16, 1);
#undef PD_LN
}

// C / ld_out of pd_layernorm, pd_layernorm_fp8 (mult = 4: a float4 per lane) and pd_layernorm_mx (mult = 32: one scale per 32 channels)
static int ln_check_args(const char* who, int C, int ld_out, int mult) {
  const bool mx = mult == 32;
  PD_CHECK_ARG(C > 0 && C % mult == 0 && C <= 256 * LN_MAXV, "%s: C=%d must be a multiple of %d%s and <= %d", who, C, mult,
               mx ? " (one scale per 32 channels)" : "", 256 * LN_MAXV);
  PD_CHECK_ARG(ld_out >= C && ld_out % mult == 0 && ld_out <= ((C + 255) / 256) * 256,
               "%s: ld_out=%d must be >= C, %smultiple of %d and within the last 256-column block", who, ld_out, mx ? "a " : "", mult);
  return PD_OK;
}

#if !PD_IS_F16
extern "C" int pd_f16_layernorm(const float*, const float*, const float*, pd_bf16*, pd_bf16*, int64_t, int, int, float, const pd_call_opts*, pd_stream_t);
extern "C" int pd_f16_patch_merge_layernorm_ex(const float*, const float*, const float*, pd_bf16*, pd_bf16*, int, int, int, int, int, int, int, int, int,
                                               float, int, const pd_call_opts*, pd_stream_t);
extern "C" int pd_f16_groupnorm_silu(const float*, const float*, const float*, const float*, const float*, int, double*, pd_bf16*, pd_bf16*, int, int,
                                     int, int, int, float, int, const pd_call_opts*, pd_stream_t);
extern "C" int pd_f16_cast_rows(const float*, pd_bf16*, pd_bf16*, int64_t, int, int, int, int, int, int, const pd_call_opts*, pd_stream_t);
#endif

extern "C" int PD_ENTRY(layernorm)(const float* x, const float* gamma, const float* beta, pd_bf16* out, pd_bf16* out_lo,
                                   int64_t rows, int C, int ld_out, float eps, const pd_call_opts* opts, pd_stream_t stream) {
  PD_FORWARD_F16(PD_OPTS_F16(opts), pd_f16_layernorm(x, gamma, beta, out, out_lo, rows, C, ld_out, eps, opts, stream));
  PD_CHECK_ARG(!PD_IS_F16 || !out_lo, "pd_layernorm: the hi/lo split exists for bfloat16 operands only");
  PD_CHECK_ARG(x && gamma && beta && out, "pd_layernorm: null pointer");
  if (const int e = ln_check_args("pd_layernorm", C, ld_out, 4)) return e;
  if (rows <= 0) return PD_OK;
  launch_layernorm<false, Out::Op16>(x, gamma, beta, out, out_lo, rows, C, ld_out, eps, 0.f, (hipStream_t)stream);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

#if !PD_IS_F16
extern "C" int pd_layernorm_fp8(const float* x, const float* gamma, const float* beta, uint8_t* out, int64_t rows, int C, int ld_out,
                                float eps, float fp8_scale, pd_stream_t stream) {
  PD_CHECK_ARG(x && gamma && beta && out && fp8_scale > 0.f, "pd_layernorm_fp8: null pointer / bad scale");
  if (const int e = ln_check_args("pd_layernorm_fp8", C, ld_out, 4)) return e;
  if (rows <= 0) return PD_OK;
  launch_layernorm<false, Out::E4M3>(x, gamma, beta, out, nullptr, rows, C, ld_out, eps, fp8_scale, (hipStream_t)stream);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// MX e4m3 rows (the A operand of pd_igemm_mx): one E8M0 scale byte per 32 channels of a row beside the payload.  A lane owns four
// consecutive channels, so a block is 8 consecutive lanes and its maximum three shuffles: no extra pass over the tensor.
extern "C" int pd_layernorm_mx(const float* x, const float* gamma, const float* beta, uint8_t* out, uint8_t* scales, int64_t rows, int C,
                               int ld_out, float eps, pd_stream_t stream) {
  PD_CHECK_ARG(x && gamma && beta && out && scales, "pd_layernorm_mx: null pointer");
  if (const int e = ln_check_args("pd_layernorm_mx", C, ld_out, 32)) return e;
  PD_CHECK_ARG((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 && ((uintptr_t)out & 3) == 0, "pd_layernorm_mx: misaligned pointer");
  if (rows <= 0) return PD_OK;
  launch_layernorm<false, Out::MX>(x, gamma, beta, out, scales, rows, C, ld_out, eps, 0.f, (hipStream_t)stream);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
#endif

extern "C" int PD_ENTRY(patch_merge_layernorm_ex)(const float* x, const float* gamma, const float* beta, pd_bf16* out, pd_bf16* out_lo,
                                                  int B, int T, int H, int W, int C, int dt, int dh, int dw, int ld_out, float eps,
                                                  int pad_nearest, const pd_call_opts* opts, pd_stream_t stream) {
  PD_FORWARD_F16(PD_OPTS_F16(opts), pd_f16_patch_merge_layernorm_ex(x, gamma, beta, out, out_lo, B, T, H, W, C, dt, dh, dw, ld_out, eps,
                                                                    pad_nearest, opts, stream));
  PD_CHECK_ARG(!PD_IS_F16 || !out_lo, "pd_patch_merge_layernorm: the hi/lo split exists for bfloat16 operands only");
  PD_CHECK_ARG(x && gamma && beta && out, "pd_patch_merge_layernorm: null pointer");
  const int Cm = C * dt * dh * dw;
  PD_CHECK_ARG((C & 3) == 0 && Cm <= 256 * LN_MAXV, "pd_patch_merge_layernorm: C=%d (merged %d) unsupported", C, Cm);
  PD_CHECK_ARG(ld_out >= Cm && (ld_out & 3) == 0 && ld_out <= ((Cm + 255) / 256) * 256, "pd_patch_merge_layernorm: bad ld_out=%d", ld_out);
  const int64_t rows = (int64_t)B * ((T + dt - 1) / dt) * ((H + dh - 1) / dh) * ((W + dw - 1) / dw);
  launch_layernorm<true, Out::Op16>(x, gamma, beta, out, out_lo, rows, Cm, ld_out, eps, 0.f, (hipStream_t)stream, T, H, W, C, dt, dh, dw,
                                    pad_nearest ? 1 : 0);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

#if !PD_IS_F16
extern "C" int pd_patch_merge_layernorm(const float* x, const float* gamma, const float* beta, pd_bf16* out, pd_bf16* out_lo,
                                        int B, int T, int H, int W, int C, int dt, int dh, int dw, int ld_out, float eps,
                                        pd_stream_t stream) {
  return pd_patch_merge_layernorm_ex(x, gamma, beta, out, out_lo, B, T, H, W, C, dt, dh, dw, ld_out, eps, 0, nullptr, stream);
}
#endif

// -------------------------------------------------------------------------------------------------
// GroupNorm on channels-last (B, S, C): pass 1 partial (sum, sumsq) per (sample, chunk of positions, group),
// pass 2 finalises mean/rstd per group in the block prologue (double), then normalise + affine [+ scale/shift]
// [+ SiLU] + bf16 cast.  Deterministic (no atomics).
// -------------------------------------------------------------------------------------------------
constexpr int GN_ROWS = 64;   // positions per stats block

#if !PD_IS_F16
extern "C" int pd_groupnorm_nchunk(int S, int C) { return (S + GN_ROWS - 1) / GN_ROWS; }
#else
extern "C" int pd_groupnorm_nchunk(int S, int C);
#endif

__global__ void __launch_bounds__(256) gn_stats_kernel(const float* __restrict__ x, double* __restrict__ partials, int S, int C,
                                                       int G) {
  // grid (nchunk, B).  Thread t walks the chunk's [rows x C] elements with stride 256; channel-fastest, so a
  // wave reads 256 contiguous bytes.  Per-group accumulation goes through LDS atomics on doubles? -> no: each thread
  // keeps (sum, sumsq) per *its* channel only when 256 % C == 0 or C % 256 == 0; the general case uses the slow path.
  extern __shared__ double sred[];   // [256][2] then [G][2]
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int r0 = chunk * GN_ROWS, r1 = min(S, r0 + GN_ROWS);
  const int cpg = C / G;
  const float* xb = x + ((int64_t)b * S + r0) * C;
  const int n = (r1 - r0) * C;
  const int tid = threadIdx.x;
  double* out = partials + ((int64_t)b * nchunk + chunk) * G * 2;
  if ((C <= 256 && 256 % C == 0) || (C % 256 == 0)) {
    // fast path: a thread always sees channels == tid (mod 256) -> one group per thread when cpg divides nicely.  The sums are fp64 from
    // the first add (x * x is exact there): gn_mean_rstd forms sumsq / n - mean^2, which multiplies the rounding of an fp32 sum of
    // squares by (mean / std)^2
    double s = 0, q = 0;
    if (C <= 256) {
      for (int i = tid; i < n; i += 256) { const double v = xb[i]; s += v; q += v * v; }
      sred[tid * 2] = s; sred[tid * 2 + 1] = q;
      __syncthreads();
      if (tid < G) {
        double ss = 0, qq = 0;
        for (int k = 0; k < 256; ++k)
          if ((k % C) / cpg == tid) { ss += sred[k * 2]; qq += sred[k * 2 + 1]; }
        out[tid * 2] = ss; out[tid * 2 + 1] = qq;
      }
    } else {
      // C multiple of 256: thread handles channels tid, tid+256, ... ; groups differ per 256-column block when cpg < 256
      const int nblk = C / 256;
      for (int k = tid; k < G * 2; k += 256) sred[512 + k] = 0.0;
      __syncthreads();
      for (int cb = 0; cb < nblk; ++cb) {
        double s2 = 0, q2 = 0;
        const int c = cb * 256 + tid;
        for (int r = 0; r < r1 - r0; ++r) { const double v = xb[(int64_t)r * C + c]; s2 += v; q2 += v * v; }
        sred[tid * 2] = s2; sred[tid * 2 + 1] = q2;
        __syncthreads();
        // groups covered by this 256-column block: [cb*256/cpg, (cb*256+255)/cpg]
        const int g0 = (cb * 256) / cpg, g1 = (cb * 256 + 255) / cpg;
        if (tid <= g1 - g0) {
          const int g = g0 + tid;
          double ss = 0, qq = 0;
          for (int k = 0; k < 256; ++k)
            if ((cb * 256 + k) / cpg == g) { ss += sred[k * 2]; qq += sred[k * 2 + 1]; }
          sred[512 + g * 2] += ss; sred[512 + g * 2 + 1] += qq;
        }
        __syncthreads();
      }
      for (int k = tid; k < G * 2; k += 256) out[k] = sred[512 + k];
    }
  } else {
    // general path (e.g. C = 65 with 65 groups): one thread per (group) walks its channels
    for (int g = tid; g < G; g += 256) {
      double ss = 0, qq = 0;
      for (int r = 0; r < r1 - r0; ++r)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) { const double v = xb[(int64_t)r * C + c]; ss += v; qq += v * v; }
      out[g * 2] = ss; out[g * 2 + 1] = qq;
    }
  }
}

// ---- (sample, group) statistics from the per-chunk fp64 partial sums [chunk][g][sum, sum of squares].  Two summation orders, each kept
// as it is (their fp64 totals, hence mean / rstd, can differ in the last bit):
//   serial   one thread walks all chunks of its group: the scalar apply kernel and pd_groupnorm_stats
//   striped  256 / G threads per group take every LP-th chunk, then one thread adds the LP sums: the vectorised apply kernel and the
//            backward pass
__device__ __forceinline__ float2 gn_mean_rstd(double sum, double sumsq, double cnt, float eps) {
  const double mean = sum / cnt;
  double var = sumsq / cnt - mean * mean;
  if (var < 0) var = 0;
  return make_float2((float)mean, (float)(1.0 / sqrt(var + (double)eps)));
}
// serial order.  pb: this sample's (nchunk, G, 2) partial sums
__device__ __forceinline__ float2 gn_stats_serial(const double* __restrict__ pb, int nchunk, int G, int g, double cnt, float eps) {
  double ss = 0, qq = 0;
  const double* pp = pb + g * 2;
  for (int k = 0; k < nchunk; ++k) { ss += pp[(int64_t)k * G * 2]; qq += pp[(int64_t)k * G * 2 + 1]; }
  return gn_mean_rstd(ss, qq, cnt, eps);
}
// striped order (G <= 256, 256 threads).  A single thread walking all the chunks is a chain of dependent L2 round trips -- 10+ us at 52
// chunks, most of an apply kernel's time at small batches; the LP strided sums are added in a fixed order (deterministic).  True for the
// threads tid < G, which hold group tid's totals; the caller stores what it derives from them and synchronises before reading it
// (or before the next call on the same spart).
__device__ __forceinline__ bool gn_reduce_partials(const double* __restrict__ pb, int nchunk, int G, double* spart, double& sum, double& sumsq) {
  const int tid = threadIdx.x, LP = 256 / G;
  if (tid < LP * G) {
    const int g = tid % G, j = tid / G;
    double a = 0, b = 0;
    for (int k = j; k < nchunk; k += LP) { a += pb[((int64_t)k * G + g) * 2]; b += pb[((int64_t)k * G + g) * 2 + 1]; }
    spart[tid * 2] = a;
    spart[tid * 2 + 1] = b;
  }
  __syncthreads();
  if (tid >= G) return false;
  sum = sumsq = 0;
  for (int j = 0; j < LP; ++j) { sum += spart[(j * G + tid) * 2]; sumsq += spart[(j * G + tid) * 2 + 1]; }
  return true;
}

__global__ void __launch_bounds__(256) gn_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ ss_scale,
                                                       const float* __restrict__ ss_shift, int ld_ss,
                                                       const double* __restrict__ partials, pd_bf16* __restrict__ out,
                                                       pd_bf16* __restrict__ out_lo, int S, int C, int G, int ld_out, float eps,
                                                       int silu, int nchunk) {
  // grid (nchunk, B): same chunking as the stats pass.
  extern __shared__ float smr[];   // [G][2] mean, rstd
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int cpg = C / G;
  const int tid = threadIdx.x;
  for (int g = tid; g < G; g += 256) {
    const float2 m = gn_stats_serial(partials + (int64_t)b * nchunk * G * 2, nchunk, G, g, (double)S * cpg, eps);
    smr[g * 2] = m.x;
    smr[g * 2 + 1] = m.y;
  }
  __syncthreads();
  const int r0 = chunk * GN_ROWS, r1 = min(S, r0 + GN_ROWS);
  const float* xb = x + ((int64_t)b * S + r0) * C;
  pd_bf16* ob = out + ((int64_t)b * S + r0) * ld_out;
  pd_bf16* obl = out_lo ? out_lo + ((int64_t)b * S + r0) * ld_out : nullptr;
  const int n = (r1 - r0) * ld_out;
  for (int i = tid; i < n; i += 256) {
    const int r = i / ld_out, c = i - r * ld_out;
    float y = 0.f;
    if (c < C) {
      const int g = c / cpg;
      y = (xb[(int64_t)r * C + c] - smr[g * 2]) * smr[g * 2 + 1] * gamma[c] + beta[c];
      if (ss_scale) y = y * (1.f + ss_scale[(int64_t)b * ld_ss + c]) + ss_shift[(int64_t)b * ld_ss + c];
      if (silu) y = y / (1.f + expf(-y));
    }
    write1(ob, obl, i, y);
  }
}

// ---- fast path: C % 4 == 0, (C/4) divides 256, channels-per-group % 4 == 0, ld_out == C.  A thread owns one float4
// column (4 channels of ONE group) and walks rows; loads are 16 B/lane, stores 8 B/lane (bf16 x4). ----
__global__ void __launch_bounds__(256) gn_stats_vec_kernel(const float* __restrict__ x, double* __restrict__ partials, int S, int C, int G) {
  __shared__ double sred[256 * 2];
  const int b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int CV = C >> 2, RP = 256 / CV;                 // float4 columns, rows per pass
  const int tid = threadIdx.x, cv = tid % CV, rr = tid / CV;
  const int r0 = chunk * GN_ROWS, r1 = min(S, r0 + GN_ROWS);
  const float4* xb = (const float4*)(x + ((int64_t)b * S + r0) * C) + cv;
  // fp64 from the first add, like gn_stats_kernel (the kernel streams HBM: a convert and two fp64 operations per element are hidden)
  double s = 0, q = 0;
#pragma unroll 4
  for (int r = rr; r < r1 - r0; r += RP) {
    const float4 v = xb[(int64_t)r * CV];
    const double v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
    s += (v0 + v1) + (v2 + v3);
    q += (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3);
  }
  sred[tid * 2] = s;
  sred[tid * 2 + 1] = q;
  __syncthreads();
  if (tid < G) {
    const int cvg = (C / G) >> 2;                       // float4 columns per group
    double ss = 0, qq = 0;
    for (int r = 0; r < RP; ++r)
      for (int k = 0; k < cvg; ++k) {
        const int t = r * CV + tid * cvg + k;
        ss += sred[t * 2];
        qq += sred[t * 2 + 1];
      }
    double* out = partials + ((int64_t)b * nchunk + chunk) * G * 2;
    out[tid * 2] = ss;
    out[tid * 2 + 1] = qq;
  }
}

// The folded affine of four channels at c: y = x * a + d with a = rstd*gamma, d = beta - mean*rstd*gamma, then (1 + scale) * y + shift of sample b
// folded in as well.  (Keep the address as base + row + c: as one 64-bit offset, gn_onepass_kernel<26, 512, 16> measured 2 % slower.)
__device__ __forceinline__ void gn_affine_fold(const float* gamma, const float* beta, int c, const float* ss_scale, const float* ss_shift,
                                               int b, int ld_ss, float mean, float rstd, float (&a)[4], float (&d)[4]) {
  const float4 ga = *(const float4*)(gamma + c), be = *(const float4*)(beta + c);
  a[0] = rstd * ga.x; a[1] = rstd * ga.y; a[2] = rstd * ga.z; a[3] = rstd * ga.w;
  d[0] = be.x - mean * a[0]; d[1] = be.y - mean * a[1]; d[2] = be.z - mean * a[2]; d[3] = be.w - mean * a[3];
  if (ss_scale) {
    const float4 sc = *(const float4*)(ss_scale + (int64_t)b * ld_ss + c), sh = *(const float4*)(ss_shift + (int64_t)b * ld_ss + c);
    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] *= (1.f + scv[k]); d[k] = d[k] * (1.f + scv[k]) + shv[k]; }
  }
}
// ... applied to a float4 [-> SiLU].  EXACT_EXP: expf instead of __expf -- the MX output, where a rounding boundary of the payload is
// 2^-4 away and the bytes are compared with a reference; every other output keeps the fast exponential.
template <bool EXACT_EXP>
__device__ __forceinline__ void gn_affine_silu4(const float4& v, const float (&a)[4], const float (&d)[4], int silu, float (&y)[4]) {
  y[0] = v.x * a[0] + d[0]; y[1] = v.y * a[1] + d[1]; y[2] = v.z * a[2] + d[2]; y[3] = v.w * a[3] + d[3];
  if (silu) {
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = y[k] / (1.f + (EXACT_EXP ? expf(-y[k]) : __expf(-y[k])));
  }
}

// OUT / out / aux / scale: see write4.  Op16 and E4M3 rows are dense (ld_out is not read); MX rows have ld_out >= C columns, and the pad
// columns [C, ld_out) get a zero payload and scale byte 0.
template <Out OUT>
__global__ void __launch_bounds__(256) gn_apply_vec_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ ss_scale,
                                                           const float* __restrict__ ss_shift, int ld_ss,
                                                           const double* __restrict__ partials, void* __restrict__ out,
                                                           void* __restrict__ aux, int S, int C, int G, int ld_out, float eps, int silu,
                                                           int nchunk, float scale) {
  __shared__ float smr[2 * 256];
  __shared__ double spart[2 * 256];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int cpg = C / G;
  const int tid = threadIdx.x;
  double ss, qq;
  if (gn_reduce_partials(partials + (int64_t)b * nchunk * G * 2, nchunk, G, spart, ss, qq)) {
    const float2 m = gn_mean_rstd(ss, qq, (double)S * cpg, eps);
    smr[tid * 2] = m.x;
    smr[tid * 2 + 1] = m.y;
  }
  __syncthreads();
  const int CV = C >> 2, RP = 256 / CV;
  const int cv = tid % CV, rr = tid / CV, c = cv * 4, g = c / cpg;
  float a[4], d[4];
  gn_affine_fold(gamma, beta, c, ss_scale, ss_shift, b, ld_ss, smr[g * 2], smr[g * 2 + 1], a, d);
  const int r0 = chunk * GN_ROWS, r1 = min(S, r0 + GN_ROWS);
  const int ld = OUT == Out::MX ? ld_out : C;
  // (MX: the 8 lanes of a block share r, C % 32 == 0.  Its loop stays rolled: its registers and time are those of the rolled form)
  constexpr int UNROLL = OUT == Out::MX ? 1 : 4;
#pragma unroll UNROLL
  for (int r = rr; r < r1 - r0; r += RP) {
    const int64_t row = (int64_t)b * S + r0 + r;
    float y[4];
    gn_affine_silu4<OUT == Out::MX>(*(const float4*)(x + row * C + c), a, d, silu, y);
    write4<OUT>(out, aux, row * ld, c, y, scale);
    if constexpr (OUT == Out::MX) {
      const int padv = (ld_out - C) >> 2;
      for (int pc = cv; pc < padv; pc += CV) {
        *(uint32_t*)((uint8_t*)out + row * ld + C + pc * 4) = 0u;
        if ((pc & 7) == 0) ((uint8_t*)aux)[(row * ld + C + pc * 4) >> 5] = 0;
      }
    }
  }
}

// ---- one pass (round 4): a workgroup owns (sample, 32 or 16 channels) and keeps its S x 32 / 16 values in registers -- statistics (two-pass in
// registers: mean, then the centred sum of squares) and the normalised bf16 rows from ONE read of x instead of two (the statistics
// kernel's pass over the tensor is gone: 109 -> 0 MB per level-0 call at 32 trajectories).  NT threads, CH = 32 or 16 channels per
// workgroup: CH / 4 threads per row segment (a float4 each), RMAX sweeps over the rows (<16, 512, 32> up to 1024 rows, <26, 512, 16> up
// to 3328: 104 data registers per thread want the 256-register budget of 8 waves); the groups of the chunk (C / G = 4, 8, 16 or 32
// channels) are reduced over the row lanes of a wave by shuffles and over the waves through LDS in a fixed order.  The choice of
// this kernel depends on the shape only, never on the batch (the engine's batch-split-reproducible mode).
template <int RMAX, int NT, int CH>
__global__ void __launch_bounds__(NT) gn_onepass_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, const float* __restrict__ ss_scale,
                                                         const float* __restrict__ ss_shift, int ld_ss, double* __restrict__ partials,
                                                         int nchunk, pd_bf16* __restrict__ out, int S, int C, int G, float eps, int silu) {
  constexpr int TPR = CH / 4, NWV = NT / 64, RP = NT / TPR;          // threads per row segment, waves, rows per sweep
  __shared__ float sred[2][NWV][TPR];
  // (sample, chunk) of this workgroup.  With 16-channel chunks a 128-byte line of a row is shared by TWO workgroups: they get ids 8
  // apart -- the same XCD (workgroups go to the XCDs round robin), next to each other in its queue -- so that the line is fetched into
  // one L2 once
  int b, chunk;
  {
    const int per_row = C / CH;
    int id = blockIdx.x;
    if (CH == 16 && id < ((int)gridDim.x & ~15)) {                     // (whole blocks of 16 ids; a tail keeps its order)
      const int h = (id >> 3) & 1, p = ((id >> 4) << 3) | (id & 7);    // pair index p, half h
      id = 2 * p + h;
    }
    b = id / per_row;
    chunk = id - b * per_row;
  }
  const int tid = threadIdx.x, slot = tid % TPR, rl = tid / TPR, wave = tid >> 6;
  const int c = chunk * CH + slot * 4, cpg = C / G, spg = cpg >> 2;   // float4 slots per group: 1, 2, 4 (or 8 with 32-channel chunks)
  // buffer addressing: the sample's rows behind one descriptor, lane offset in a VGPR, the sweep's offset in an SGPR -- no per-load
  // address registers (35 in-flight 64-bit pointers were what spilled); rows >= S get an out-of-range lane offset: zeros / dropped stores
  const auto rX = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (int64_t)b * S * C), 0, (uint32_t)((int64_t)S * C * 4), 0x00020000);
  const auto rO = __builtin_amdgcn_make_buffer_rsrc((void*)(out + (int64_t)b * S * C), 0, (uint32_t)((int64_t)S * C * 2), 0x00020000);
  const uint32_t voff = (uint32_t)(rl * C + c) * 4u, sstep = (uint32_t)(RP * C) * 4u;
  constexpr uint32_t GN_OOB = 0xFFFFF000u;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2_t;
  float4 v[RMAX];
#pragma unroll
  for (int i = 0; i < RMAX; ++i) {
    // rows >= S: an out-of-range LANE offset (whether the hardware's range check also counts the scalar offset is not relied upon)
    const u32x4_t w = __builtin_amdgcn_raw_buffer_load_b128(rX, rl + RP * i < S ? voff : GN_OOB, (uint32_t)i * sstep, 0);
    v[i] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
  }
  // sum over the workgroup's values of this thread's group: row lanes of the wave (lane bits 3..5), the group's slots (lane bits
  // 0..log2(spg)-1), then the 8 waves in order
  auto group_sum = [&](float t, int buf) {
#pragma unroll
    for (int m = TPR; m < 64; m <<= 1) t += __shfl_xor(t, m);
    for (int m = 1; m < spg; m <<= 1) t += __shfl_xor(t, m);
    if ((tid & 63) < TPR) sred[buf][wave][slot] = t;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) tot += sred[buf][w][slot];
    return tot;
  };
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < RMAX; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float cnt = (float)S * (float)cpg;
  const float mean = group_sum(s, 0) / cnt;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < RMAX; ++i) {
    if (rl + RP * i < S) {
      const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  const float var = group_sum(q, 1) / cnt;
  const float rstd = 1.0f / sqrtf(var + eps);
  // `partials` keeps its contract -- the (sample, group)'s statistics as fp64 partial sums [b][chunk][g][sum, sum of squares], which
  // pd_groupnorm_silu_bwd reduces again: everything in chunk 0 (mean * n and (var + mean^2) * n reproduce this kernel's mean and
  // variance exactly in fp64), zeros in the others
  if (rl == 0 && slot % spg == 0) {
    double* pp = partials + (int64_t)b * nchunk * G * 2 + (c / cpg) * 2;
    pp[0] = (double)mean * (double)cnt;
    pp[1] = ((double)var + (double)mean * (double)mean) * (double)cnt;
    for (int k = 1; k < nchunk; ++k) { pp[(int64_t)k * G * 2] = 0.0; pp[(int64_t)k * G * 2 + 1] = 0.0; }
  }
  float a[4], d[4];
  gn_affine_fold(gamma, beta, c, ss_scale, ss_shift, b, ld_ss, mean, rstd, a, d);
#pragma unroll
  for (int i = 0; i < RMAX; ++i) {
    float y[4];
    gn_affine_silu4<false>(v[i], a, d, silu, y);
    const uint2 p = pack_op4(y);
    const u32x2_t o = {p.x, p.y};
    __builtin_amdgcn_raw_buffer_store_b64(o, rO, rl + RP * i < S ? voff >> 1 : GN_OOB, ((uint32_t)i * sstep) >> 1, 0);
    if ((i & 1) == 1) __builtin_amdgcn_sched_barrier(0);      // (two rows at a time: an unbounded interleave of the 35 rows spilled)
  }
}

// Shapes of the one-pass kernel: 16-channel chunks holding whole groups, at most 26 x 128 rows (everything of a (sample, chunk) in registers)
static bool gn_onepass_fits(int S, int C, int G) {
  const int cpg = C / G;
  return C % 32 == 0 && cpg % 4 == 0 && 16 % cpg == 0 && S <= 128 * 26;
}
// `fine` (pd_call_opts.small_grid: the caller may choose kernels by launch size -- the engine's small-batch mode) at <= 1024 rows, when the
// 32-channel chunks would leave more than half of the CUs without a workgroup: 16-channel chunks, twice the workgroups, half the rows in
// flight per thread (level-1 rows of the SEVIR-LR denoiser at 4 trajectories: 7.3 vs 9.3 us).  Its statistics are summed in another order
// than the coarse kernel's (not bit-identical to it).  Not for the longer rows: 8-channel chunks there read 32 B of every 128-B line
// (measured 17.8 vs 16.7 us at level 0).
static void gn_onepass_launch(const float* x, const float* gamma, const float* beta, const float* ss_scale, const float* ss_shift, int ld_ss,
                              double* partials, int nchunk, pd_bf16* out, int B, int S, int C, int G, float eps, int silu, bool fine,
                              hipStream_t s) {
  const int cpg = C / G;
  const bool small = S <= 64 * 16;
  fine = fine && small && 16 % cpg == 0 && (int64_t)B * (C / 32) * 2 <= pd_num_cus();
#define GN1P(RM, CHN) hipLaunchKernelGGL((gn_onepass_kernel<RM, 512, CHN>), dim3(B * (C / CHN)), dim3(512), 0, s, x, gamma, beta, ss_scale, ss_shift, \
                                         ld_ss, partials, nchunk, out, S, C, G, eps, silu)
  if (small) { if (fine) GN1P(8, 16); else GN1P(16, 32); }
  else GN1P(26, 16);
#undef GN1P
}

// ---- one pass for narrow rows whose channel count the kernels above cannot take (the stem of the denoiser: C = 65, one group per channel;
// before: the scalar statistics + apply pair of launches).  A workgroup owns (sample, up to 16 channels holding whole groups) and keeps its
// S x 16 values in registers, one per (row lane, channel slot) and sweep: 32 rows per sweep, RMAX sweeps (104: up to 3328 rows).  Rows are
// not 16 B aligned (C is odd), so the loads are single dwords through a buffer descriptor (no address registers per load; rows >= S and
// the slots past the workgroup's channels get an out-of-range lane offset: zeros).  Statistics in the one-pass kernel's form -- fp32 mean,
// then the centred sum of squares -- reduced over the four row lanes of a wave by shuffles, then over the waves and the group's slots
// through LDS in a fixed order.  `partials` as gn_onepass_kernel writes it.  The pad columns [C, ld_out) are zeroed, each of the
// sample's workgroups taking every nsplit-th row.
template <int RMAX>
__global__ void __launch_bounds__(512) gn_narrow_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ ss_scale,
                                                        const float* __restrict__ ss_shift, int ld_ss, double* __restrict__ partials,
                                                        int nchunk, pd_bf16* __restrict__ out, int S, int C, int G, int ld_out, float eps,
                                                        int silu, int gpw, int nsplit) {
  constexpr int NWV = 8, RP = 32;
  __shared__ float sred[2][NWV][16];
  const int b = blockIdx.x / nsplit, part = blockIdx.x - b * nsplit;
  const int cpg = C / G;
  const int g0 = part * gpw, g1 = min(G, g0 + gpw);
  const int c0 = g0 * cpg, nch = (g1 - g0) * cpg;                    // this workgroup's channels: [c0, c0 + nch), nch <= 16
  const int tid = threadIdx.x, slot = tid & 15, rl = tid >> 4, wave = tid >> 6;
  const bool active = slot < nch;
  const int c = c0 + (active ? slot : 0);
  const int gl = (active ? slot : 0) / cpg;                          // the thread's group, local
  const auto rX = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (int64_t)b * S * C), 0, (uint32_t)((int64_t)S * C * 4), 0x00020000);
  const uint32_t voff = (uint32_t)(rl * C + c) * 4u, sstep = (uint32_t)(RP * C) * 4u;
  constexpr uint32_t GN_OOB = 0xFFFFF000u;
  float v[RMAX];
#pragma unroll
  for (int i = 0; i < RMAX; ++i)
    v[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rX, (active && rl + RP * i < S) ? voff : GN_OOB, (uint32_t)i * sstep, 0));
  auto group_sum = [&](float t, int buf) {
    t += __shfl_xor(t, 16);
    t += __shfl_xor(t, 32);
    if ((tid & 63) < 16) sred[buf][wave][slot] = t;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < NWV; ++w)
      for (int k = 0; k < cpg; ++k) tot += sred[buf][w][gl * cpg + k];
    return tot;
  };
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < RMAX; ++i) s += v[i];
  const float cnt = (float)S * (float)cpg;
  const float mean = group_sum(s, 0) / cnt;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < RMAX; ++i) {
    if (rl + RP * i < S) {
      const float d0 = v[i] - mean;
      q += d0 * d0;
    }
  }
  const float var = group_sum(active ? q : 0.f, 1) / cnt;
  const float rstd = 1.0f / sqrtf(var + eps);
  if (active && rl == 0 && slot % cpg == 0) {
    double* pp = partials + (int64_t)b * nchunk * G * 2 + (g0 + gl) * 2;
    pp[0] = (double)mean * (double)cnt;
    pp[1] = ((double)var + (double)mean * (double)mean) * (double)cnt;
    for (int k = 1; k < nchunk; ++k) { pp[(int64_t)k * G * 2] = 0.0; pp[(int64_t)k * G * 2 + 1] = 0.0; }
  }
  float a = 0.f, d = 0.f;
  if (active) {
    a = rstd * gamma[c];
    d = beta[c] - mean * a;
    if (ss_scale) {
      const float sc = ss_scale[(int64_t)b * ld_ss + c], sh = ss_shift[(int64_t)b * ld_ss + c];
      a *= (1.f + sc);
      d = d * (1.f + sc) + sh;
    }
  }
  pd_bf16* ob = out + (int64_t)b * S * ld_out;
#pragma unroll
  for (int i = 0; i < RMAX; ++i) {
    const int r = rl + RP * i;
    float y = v[i] * a + d;
    if (silu) y = y / (1.f + __expf(-y));
    if (active && r < S) ob[(int64_t)r * ld_out + c] = f2op(y);
  }
  const int npad = ld_out - C;
  if (npad > 0) {
    const int rows = (S - part + nsplit - 1) / nsplit;               // rows part, part + nsplit, ...
    for (int i = tid; i < rows * npad; i += 512) {
      const int j = i / npad, pc = i - j * npad;
      ob[(int64_t)(part + j * nsplit) * ld_out + C + pc] = 0;
    }
  }
}
// Shapes of the narrow one-pass kernel: what the vectorised kernels refuse, rows of at most 128 channels, groups of at most 16, at most
// 104 x 32 rows -- and at least 8 x 32: a sample of fewer rows leaves most of the 512 threads' sweeps empty (70 rows: three sweeps, the
// third a fifth full), there the statistics + apply pair stays
static bool gn_narrow_fits(int S, int C, int G) { return C <= 128 && C / G <= 16 && S >= 32 * 8 && S <= 32 * 104; }
static void gn_narrow_launch(const float* x, const float* gamma, const float* beta, const float* ss_scale, const float* ss_shift, int ld_ss,
                             double* partials, int nchunk, pd_bf16* out, int B, int S, int C, int G, int ld_out, float eps, int silu,
                             hipStream_t s) {
  const int cpg = C / G;
  const int nsplit = (G + 16 / cpg - 1) / (16 / cpg), gpw = (G + nsplit - 1) / nsplit;   // workgroups per sample, evenly filled (65 groups of one: 5 x 13)
#define GNNR(RM) hipLaunchKernelGGL((gn_narrow_kernel<RM>), dim3(B * nsplit), dim3(512), 0, s, x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, \
                                    nchunk, out, S, C, G, ld_out, eps, silu, gpw, nsplit)
  if (S <= 32 * 26) GNNR(26);
  else GNNR(104);
#undef GNNR
}

// Shapes and pointers of the vectorised kernels (gn_stats_vec_kernel, gn_apply_vec_kernel): a thread owns one float4 column of ONE group,
// 256 threads hold whole rows.  gamma / beta / scale-shift may be null where the caller has none.  The output's own conditions (alignment
// of its packed store, dense rows) are the caller's.
static bool gn_vec_ok(int C, int G, const float* x, const float* gamma, const float* beta, const float* ss_scale, const float* ss_shift,
                      int ld_ss) {
  if (C % 4 != 0) return false;
  const int CV = C / 4, cpg = C / G;
  return CV <= 256 && (256 % CV == 0) && (cpg % 4 == 0) && G <= 256 && (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0 &&
         (!ss_scale || ((ld_ss % 4 == 0) && (((uintptr_t)ss_scale | (uintptr_t)ss_shift) & 15) == 0));
}

// The two launches (statistics, apply) behind pd_groupnorm_silu's vectorised branch, pd_groupnorm_silu_fp8 and pd_groupnorm_silu_mx
template <Out OUT>
static int gn_two_pass(const float* x, const float* gamma, const float* beta, const float* ss_scale, const float* ss_shift, int ld_ss,
                       double* partials, void* out, void* aux, int B, int S, int C, int G, int ld_out, float eps, int silu, float scale,
                       hipStream_t s) {
  const int nchunk = pd_groupnorm_nchunk(S, C);
  hipLaunchKernelGGL(gn_stats_vec_kernel, dim3(nchunk, B), dim3(256), 0, s, x, partials, S, C, G);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_apply_vec_kernel<OUT>, dim3(nchunk, B), dim3(256), 0, s, x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, out, aux,
                     S, C, G, ld_out, eps, silu, nchunk, scale);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int PD_ENTRY(groupnorm_silu)(const float* x, const float* gamma, const float* beta, const float* ss_scale,
                                        const float* ss_shift, int ld_ss, double* partials, pd_bf16* out, pd_bf16* out_lo, int B, int S,
                                        int C, int G, int ld_out, float eps, int silu, const pd_call_opts* opts, pd_stream_t stream) {
  PD_FORWARD_F16(PD_OPTS_F16(opts), pd_f16_groupnorm_silu(x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, out, out_lo, B, S, C, G, ld_out,
                                                          eps, silu, opts, stream));
  PD_CHECK_ARG(!PD_IS_F16 || !out_lo, "pd_groupnorm_silu: the hi/lo split exists for bfloat16 operands only");
  const bool onepass = !(opts && opts->groupnorm_two_launches);      // A/B: the statistics + apply pair of launches instead of the one-pass kernel
  PD_CHECK_ARG(x && gamma && beta && partials && out, "pd_groupnorm_silu: null pointer");
  PD_CHECK_ARG(G > 0 && C % G == 0 && ld_out >= C, "pd_groupnorm_silu: bad C/G/ld_out (%d,%d,%d)", C, G, ld_out);
  PD_CHECK_ARG((ss_scale == nullptr) == (ss_shift == nullptr), "pd_groupnorm_silu: scale/shift must come together");
  PD_CHECK_ARG(G <= 4096, "pd_groupnorm_silu: too many groups");
  const int nchunk = pd_groupnorm_nchunk(S, C);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = gn_vec_ok(C, G, x, gamma, beta, ss_scale, ss_shift, ld_ss) && ld_out == C && (((uintptr_t)out | (uintptr_t)out_lo) & 7) == 0;
  // bf16 engine (no lo half), 16-channel chunks holding whole groups, at most 26 x 128 rows: everything of a (sample, chunk) in registers
  if (vec && onepass && !out_lo && gn_onepass_fits(S, C, G)) {
    gn_onepass_launch(x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, nchunk, out, B, S, C, G, eps, silu,
                      opts && opts->small_grid, s);
    PD_CHECK_LAUNCH();
    return PD_OK;
  }
  if (vec) return gn_two_pass<Out::Op16>(x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, out, out_lo, B, S, C, G, ld_out, eps, silu, 1.f, s);
  // narrow rows the vectorised kernels cannot take (C = 65: the stem), bf16 engine: one launch, everything of a (sample, 16 channels) in registers
  if (onepass && !out_lo && gn_narrow_fits(S, C, G)) {
    gn_narrow_launch(x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, nchunk, out, B, S, C, G, ld_out, eps, silu, s);
    PD_CHECK_LAUNCH();
    return PD_OK;
  }
  hipLaunchKernelGGL(gn_stats_kernel, dim3(nchunk, B), dim3(256), (512 + 2 * G) * sizeof(double), s, x, partials, S, C, G);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_apply_kernel, dim3(nchunk, B), dim3(256), 2 * G * sizeof(float), s, x, gamma, beta, ss_scale, ss_shift,
                     ld_ss, partials, out, out_lo, S, C, G, ld_out, eps, silu, nchunk);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// Statistics only: mean / rstd per (sample, group) as fp32 pairs from the same fp64 partial sums, the chunks summed serially: the order
// of gn_apply_kernel's prologue (the vectorised apply kernel stripes the chunks, so its own mean / rstd may differ from these in the last
// bit) -- for consumers that normalise on the fly (pd_conv2d_gn_silu: the VAE's fused ResBlock convolution).
__global__ void __launch_bounds__(256) gn_finalize_kernel(const double* __restrict__ partials, float* __restrict__ stats, int S, int C, int G,
                                                          int nchunk, float eps) {
  const int b = blockIdx.x;
  const int cpg = C / G;
  for (int g = threadIdx.x; g < G; g += 256) {
    const float2 m = gn_stats_serial(partials + (int64_t)b * nchunk * G * 2, nchunk, G, g, (double)S * cpg, eps);
    stats[((int64_t)b * G + g) * 2] = m.x;
    stats[((int64_t)b * G + g) * 2 + 1] = m.y;
  }
}

#if !PD_IS_F16
extern "C" int pd_groupnorm_stats(const float* x, double* partials, float* stats, int B, int S, int C, int G, float eps, pd_stream_t stream) {
  PD_CHECK_ARG(x && partials && stats, "pd_groupnorm_stats: null pointer");
  PD_CHECK_ARG(G > 0 && C % G == 0 && G <= 4096 && B > 0 && S > 0, "pd_groupnorm_stats: bad B/S/C/G (%d,%d,%d,%d)", B, S, C, G);
  const int nchunk = pd_groupnorm_nchunk(S, C);
  hipStream_t s = (hipStream_t)stream;
  if (gn_vec_ok(C, G, x, nullptr, nullptr, nullptr, nullptr, 0)) hipLaunchKernelGGL(gn_stats_vec_kernel, dim3(nchunk, B), dim3(256), 0, s, x, partials, S, C, G);
  else hipLaunchKernelGGL(gn_stats_kernel, dim3(nchunk, B), dim3(256), (512 + 2 * G) * sizeof(double), s, x, partials, S, C, G);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(B), dim3(256), 0, s, partials, stats, S, C, G, nchunk, eps);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// GroupNorm [-> SiLU] -> e4m3 rows (the operand of an fp8 pd_igemm launch): out[b, s, c] = e4m3(y * fp8_scale), ld_out == C
extern "C" int pd_groupnorm_silu_fp8(const float* x, const float* gamma, const float* beta, const float* ss_scale,
                                     const float* ss_shift, int ld_ss, double* partials, uint8_t* out, int B, int S, int C, int G,
                                     float eps, int silu, float fp8_scale, pd_stream_t stream) {
  PD_CHECK_ARG(x && gamma && beta && partials && out, "pd_groupnorm_silu_fp8: null pointer");
  PD_CHECK_ARG(G > 0 && C % G == 0 && fp8_scale > 0.f, "pd_groupnorm_silu_fp8: bad C/G/scale (%d,%d,%g)", C, G, (double)fp8_scale);
  PD_CHECK_ARG((ss_scale == nullptr) == (ss_shift == nullptr), "pd_groupnorm_silu_fp8: scale/shift must come together");
  if (!(gn_vec_ok(C, G, x, gamma, beta, ss_scale, ss_shift, ld_ss) && ((uintptr_t)out & 3) == 0)) {
    pd_set_error("pd_groupnorm_silu_fp8: needs C %% 4 == 0, C/4 dividing 256 and 4 | C/G (C = %d, G = %d)", C, G);
    return PD_ERR_UNSUPPORTED;
  }
  return gn_two_pass<Out::E4M3>(x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, out, nullptr, B, S, C, G, C, eps, silu, fp8_scale,
                                (hipStream_t)stream);
}

// GroupNorm [-> scale-shift] [-> SiLU] -> MX e4m3 rows (the A operand of a pd_igemm_mx convolution); columns [C, ld_out) are padding
extern "C" int pd_groupnorm_silu_mx(const float* x, const float* gamma, const float* beta, const float* ss_scale, const float* ss_shift,
                                    int ld_ss, double* partials, uint8_t* out, uint8_t* scales, int B, int S, int C, int G, int ld_out,
                                    float eps, int silu, pd_stream_t stream) {
  PD_CHECK_ARG(x && gamma && beta && partials && out && scales, "pd_groupnorm_silu_mx: null pointer");
  PD_CHECK_ARG(G > 0 && C % G == 0 && (C & 31) == 0, "pd_groupnorm_silu_mx: bad C/G (%d,%d): C must be a multiple of 32 (one scale per 32 channels)", C, G);
  PD_CHECK_ARG(ld_out >= C && (ld_out & 31) == 0 && ld_out - C < 128, "pd_groupnorm_silu_mx: ld_out=%d must be a multiple of 32 in [C, C + 128)", ld_out);
  PD_CHECK_ARG((ss_scale == nullptr) == (ss_shift == nullptr), "pd_groupnorm_silu_mx: scale/shift must come together");
  if (!(gn_vec_ok(C, G, x, gamma, beta, ss_scale, ss_shift, ld_ss) && ((uintptr_t)out & 3) == 0)) {
    pd_set_error("pd_groupnorm_silu_mx: needs C/4 dividing 256 and 4 | C/G (C = %d, G = %d)", C, G);
    return PD_ERR_UNSUPPORTED;
  }
  return gn_two_pass<Out::MX>(x, gamma, beta, ss_scale, ss_shift, ld_ss, partials, out, scales, B, S, C, G, ld_out, eps, silu, 0.f,
                              (hipStream_t)stream);
}

// -------------------------------------------------------------------------------------------------
// Data gradient of y = SiLU(GroupNorm(x)) on channels-last rows (guidance network, frozen affine): with xh = (x - mean) rstd,
// n = gamma xh + beta, dn = dy SiLU'(n), dxh = dn gamma and N = S * C/G elements per (sample, group):
//   dx = rstd (dxh - mean_N(dxh) - xh mean_N(dxh xh)).
// Two passes like the forward: per-chunk fp64 partial sums of (dxh, dxh xh), then the apply pass reduces them in a fixed order
// (deterministic).  mean / rstd are re-derived from the forward's partial sums.  A thread owns one channel; C divides 256.
// -------------------------------------------------------------------------------------------------
template <bool APPLY>
__global__ void __launch_bounds__(256) gn_silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const double* __restrict__ fwd_partials, double* __restrict__ bwd_partials,
                                                          float* __restrict__ dx, int S, int C, int G, float eps, int silu, int nchunk) {
  __shared__ double spart[2 * 256];
  __shared__ double sfwd[2 * 256];
  __shared__ double sbwd[2 * 256];
  __shared__ float sred[2 * 256];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int cpg = C / G;
  const double cnt = (double)S * cpg;
  double t1, t2;
  if (gn_reduce_partials(fwd_partials + (int64_t)b * nchunk * G * 2, nchunk, G, spart, t1, t2)) { sfwd[tid * 2] = t1; sfwd[tid * 2 + 1] = t2; }
  __syncthreads();
  if (APPLY) {
    if (gn_reduce_partials(bwd_partials + (int64_t)b * nchunk * G * 2, nchunk, G, spart, t1, t2)) { sbwd[tid * 2] = t1; sbwd[tid * 2 + 1] = t2; }
    __syncthreads();
  }
  const int c = tid % C, rr = tid / C, RP = 256 / C, g = c / cpg;
  const float2 mr = gn_mean_rstd(sfwd[g * 2], sfwd[g * 2 + 1], cnt, eps);
  const float mean = mr.x, rstd = mr.y;
  // n from the centred xh, not from the folded x * (rstd gamma) + (beta - mean rstd gamma): the fold rounds at |mean| rstd, which on a
  // near-constant group (rstd up to 1 / sqrt(eps)) is 1e-4 of n, the same way in every row -- it adds up in the partial sums
  const float ga = gamma[c], be = beta[c];
  const float m1 = APPLY ? (float)(sbwd[g * 2] / cnt) : 0.f, m2 = APPLY ? (float)(sbwd[g * 2 + 1] / cnt) : 0.f;
  const int r0 = chunk * GN_ROWS, r1 = min(S, r0 + GN_ROWS);
  const int64_t base = ((int64_t)b * S + r0) * C + c;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll 4
  for (int r = rr; r < r1 - r0; r += RP) {
    const float xv = x[base + (int64_t)r * C], gy = dy[base + (int64_t)r * C];
    const float xh = (xv - mean) * rstd, n = xh * ga + be;
    float dn = gy;
    if (silu) {
      const float sig = 1.f / (1.f + __expf(-n));
      dn = gy * sig * (1.f + n * (1.f - sig));
    }
    const float dxh = dn * ga;
    if (APPLY) {
      dx[base + (int64_t)r * C] = rstd * (dxh - m1 - xh * m2);
    } else {
      s1 += dxh;
      s2 += dxh * xh;
    }
  }
  if (!APPLY) {
    sred[tid * 2] = s1;
    sred[tid * 2 + 1] = s2;
    __syncthreads();
    if (tid < G) {
      double a1 = 0, a2 = 0;
      for (int r = 0; r < RP; ++r)
        for (int k = 0; k < cpg; ++k) {
          const int t = r * C + tid * cpg + k;
          a1 += sred[t * 2];
          a2 += sred[t * 2 + 1];
        }
      double* out = bwd_partials + ((int64_t)b * nchunk + chunk) * G * 2;
      out[tid * 2] = a1;
      out[tid * 2 + 1] = a2;
    }
  }
}

extern "C" int pd_groupnorm_silu_bwd(const float* x, const float* dy, const float* gamma, const float* beta,
                                     const double* fwd_partials, double* bwd_partials, float* dx, int B, int S, int C, int G,
                                     float eps, int silu, pd_stream_t stream) {
  PD_CHECK_ARG(x && dy && gamma && beta && fwd_partials && bwd_partials && dx, "pd_groupnorm_silu_bwd: null pointer");
  PD_CHECK_ARG(G > 0 && C % G == 0, "pd_groupnorm_silu_bwd: bad C/G (%d,%d)", C, G);
  if (C > 256 || 256 % C != 0 || G > 256) {
    pd_set_error("pd_groupnorm_silu_bwd: C = %d must divide 256 (G = %d <= 256)", C, G);
    return PD_ERR_UNSUPPORTED;
  }
  if (B <= 0 || S <= 0) return PD_OK;
  const int nchunk = pd_groupnorm_nchunk(S, C);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gn_silu_bwd_kernel<false>, dim3(nchunk, B), dim3(256), 0, s, x, dy, gamma, beta, fwd_partials, bwd_partials, dx, S, C, G,
                     eps, silu, nchunk);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_silu_bwd_kernel<true>, dim3(nchunk, B), dim3(256), 0, s, x, dy, gamma, beta, fwd_partials, bwd_partials, dx, S, C, G,
                     eps, silu, nchunk);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

#endif   // !PD_IS_F16 (statistics-only, e4m3 and backward entry points: one copy, in the bf16 build)

// -------------------------------------------------------------------------------------------------
// fp32 -> bf16 row cast with row-slice gather and zero column padding
// -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cast_rows_kernel(const float* __restrict__ x, pd_bf16* __restrict__ out,
                                                        pd_bf16* __restrict__ out_lo, int64_t n_out_rows, int rows_in, int row_off,
                                                        int rows_out, int C, int ld_in, int ld_out) {
  const int64_t total = n_out_rows * ld_out;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ro = i / ld_out;
    const int c = (int)(i - ro * ld_out);
    const int64_t smp = ro / rows_out;
    const int r = (int)(ro - smp * rows_out);
    const float v = c < C ? x[(smp * rows_in + row_off + r) * (int64_t)ld_in + c] : 0.f;
    write1(out, out_lo, i, v);
  }
}

// ... four columns per thread (16 B loads, 8 B stores) where the rows allow it: C, ld_in, ld_out multiples of 4, no low halves.  The same
// round-to-nearest-even values as the scalar kernel's (which moves 2 B per lane and divides twice per element: 29 us for the 50 MB of the
// denoiser's head input, six times the time its bytes need).
__global__ void __launch_bounds__(256) cast_rows_vec_kernel(const float* __restrict__ x, pd_bf16* __restrict__ out, int64_t n_out_rows, int rows_in,
                                                            int row_off, int rows_out, int C, int ld_in, int ld_out) {
  const int lv = ld_out >> 2;
  const int64_t total = n_out_rows * lv;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t ro = i / lv;
    const int c = (int)(i - ro * lv) * 4;
    const int64_t smp = ro / rows_out;
    const int r = (int)(ro - smp * rows_out);
    float y[4] = {0.f, 0.f, 0.f, 0.f};
    if (c < C) {
      const float4 v = *(const float4*)(x + (smp * rows_in + row_off + r) * (int64_t)ld_in + c);
      y[0] = v.x; y[1] = v.y; y[2] = v.z; y[3] = v.w;
    }
    *(uint2*)(out + ro * ld_out + c) = pack_op4(y);
  }
}

extern "C" int PD_ENTRY(cast_rows)(const float* x, pd_bf16* out, pd_bf16* out_lo, int64_t n_samples, int rows_per_sample_in, int row_off,
                                   int rows_per_sample_out, int C, int ld_in, int ld_out, const pd_call_opts* opts, pd_stream_t stream) {
  PD_FORWARD_F16(PD_OPTS_F16(opts), pd_f16_cast_rows(x, out, out_lo, n_samples, rows_per_sample_in, row_off, rows_per_sample_out, C, ld_in,
                                                     ld_out, opts, stream));
  PD_CHECK_ARG(!PD_IS_F16 || !out_lo, "pd_cast_rows: the hi/lo split exists for bfloat16 operands only");
  PD_CHECK_ARG(x && out, "pd_cast_rows: null pointer");
  PD_CHECK_ARG(row_off >= 0 && row_off + rows_per_sample_out <= rows_per_sample_in && ld_in >= C && ld_out >= C, "pd_cast_rows: bad geometry");
  const int64_t rows = n_samples * rows_per_sample_out;
  if (rows <= 0) return PD_OK;
  const int64_t total = rows * ld_out;
  if (!out_lo && ((C | ld_in | ld_out) & 3) == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 7) == 0) {
    const unsigned gridv = (unsigned)min((int64_t)8192, (total / 4 + 255) / 256);
    hipLaunchKernelGGL(cast_rows_vec_kernel, dim3(gridv), dim3(256), 0, (hipStream_t)stream, x, out, rows, rows_per_sample_in, row_off,
                       rows_per_sample_out, C, ld_in, ld_out);
    PD_CHECK_LAUNCH();
    return PD_OK;
  }
  const unsigned grid = (unsigned)min((int64_t)4096, (total + 255) / 256);
  hipLaunchKernelGGL(cast_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, out, out_lo, rows, rows_per_sample_in, row_off,
                     rows_per_sample_out, C, ld_in, ld_out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}


}  // namespace PD_NS
