// Small HBM-bound glue kernels of the sampling path + error plumbing of the C ABI.
#include <stdarg.h>
#include "common.h"

static thread_local char g_err[512] = "";
extern "C" void pd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* pd_last_error(void) { return g_err; }
extern "C" int pd_abi_version(void) { return 4; }   // 2: per-call options (pd_call_opts), IEEE-half operand builds, no exported data symbols; 3: pd_call_opts.small_grid; 4: pd_cuboid_attn_args.qkv_fp8_log2 (was reserved); (pd_igemm_args.rowtab at the tail: pd_sizeof_igemm_args tells a stale binding)
extern "C" int pd_sizeof_igemm_args(void) { return (int)sizeof(pd_igemm_args); }
extern "C" int pd_sizeof_cuboid_attn_args(void) { return (int)sizeof(pd_cuboid_attn_args); }
extern "C" int pd_sizeof_call_opts(void) { return (int)sizeof(pd_call_opts); }
extern "C" int pd_sizeof_mx_operands(void) { return (int)sizeof(pd_mx_operands); }

static inline unsigned grid_for(int64_t n) { return (unsigned)min((int64_t)8192, (n + 255) / 256); }

// ---- cat([cond, x], T) + observation indicator channel (cuboid_transformer_unet.py:425-428) ----
__global__ void __launch_bounds__(256) build_input_kernel(const float* __restrict__ x, const float* __restrict__ cond,
                                                          float* __restrict__ out, int B, int T_in, int T_out, int HW, int C, int ld_out) {
  const int T = T_in + T_out;
  const int64_t total = (int64_t)B * T * HW * ld_out;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % ld_out);
    const int64_t pos = i / ld_out;
    const int s = (int)(pos % HW);
    const int t = (int)((pos / HW) % T);
    const int64_t b = pos / ((int64_t)HW * T);
    float v = 0.f;
    if (c < C)
      v = t < T_in ? cond[((b * T_in + t) * HW + s) * C + c] : x[((b * T_out + (t - T_in)) * HW + s) * C + c];
    else if (c == C)
      v = t < T_in ? 1.f : 0.f;
    out[i] = v;
  }
}
extern "C" int pd_unet_build_input(const float* x, const float* cond, float* out, int B, int T_in, int T_out, int HW, int C, int ld_out,
                                   pd_stream_t stream) {
  PD_CHECK_ARG(x && cond && out && ld_out >= C + 1, "pd_unet_build_input: bad args");
  const int64_t total = (int64_t)B * (T_in + T_out) * HW * ld_out;
  hipLaunchKernelGGL(build_input_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, cond, out, B, T_in, T_out, HW, C, ld_out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ... and, in the same pass, the bfloat16 copy of those rows that the stem's skip convolution reads (rows of ld16 elements, zero padded):
// what pd_cast_rows made of `out` in a launch of its own.  A thread moves four channels of one position (16 B loads; the fp32 rows of
// C + 1 elements are not 16 B aligned: four dword stores) and the four pad columns C + 4 j .. of the 16-bit row, the first of which is
// the indicator.
__global__ void __launch_bounds__(256) build_input16_kernel(const float* __restrict__ x, const float* __restrict__ cond, float* __restrict__ out,
                                                            uint16_t* __restrict__ out16, int B, int T_in, int T_out, int HW, int C, int ld_out,
                                                            int ld16) {
  const int T = T_in + T_out, CV = C >> 2;
  const int64_t total = (int64_t)B * T * HW * CV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int j = (int)(i % CV);
    const int64_t pos = i / CV;
    const int s = (int)(pos % HW);
    const int t = (int)((pos / HW) % T);
    const int64_t b = pos / ((int64_t)HW * T);
    const float4 v = t < T_in ? *(const float4*)(cond + ((b * T_in + t) * HW + s) * C + 4 * j)
                              : *(const float4*)(x + ((b * T_out + (t - T_in)) * HW + s) * C + 4 * j);
    const float ind = t < T_in ? 1.f : 0.f;
    float* o = out + pos * ld_out;
    o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
    if (j == 0) {
      o[C] = ind;
      for (int c = C + 1; c < ld_out; ++c) o[c] = 0.f;
    }
    uint16_t* o16 = out16 + pos * ld16;
    *(uint2*)(o16 + 4 * j) = make_uint2(pack_op2(v.x, v.y), pack_op2(v.z, v.w));
    if (C + 4 * j < ld16) *(uint2*)(o16 + C + 4 * j) = make_uint2(j == 0 ? pack_op2(ind, 0.f) : 0u, 0u);
  }
}
extern "C" int pd_unet_build_input16(const float* x, const float* cond, float* out, pd_bf16* out16, int B, int T_in, int T_out, int HW, int C,
                                     int ld_out, int ld16, pd_stream_t stream) {
  PD_CHECK_ARG(x && cond && out && out16 && ld_out >= C + 1, "pd_unet_build_input16: bad args");
  PD_CHECK_ARG(C > 0 && (C & 3) == 0 && (ld16 & 3) == 0 && ld16 >= C + 1 && ld16 <= 2 * C,
               "pd_unet_build_input16: C (%d) must be a multiple of 4 and ld16 (%d) one in (C, 2 C]", C, ld16);
  PD_CHECK_ARG((((uintptr_t)x | (uintptr_t)cond) & 15) == 0 && ((uintptr_t)out16 & 7) == 0, "pd_unet_build_input16: x / cond must be 16 B aligned, out16 8 B");
  const int64_t total = (int64_t)B * (T_in + T_out) * HW * (C >> 2);
  hipLaunchKernelGGL(build_input16_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, cond, out, out16, B, T_in, T_out, HW, C,
                     ld_out, ld16);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- sinusoidal timestep embedding, [cos | sin] (models/utils.py:68-88) ----
__global__ void timestep_embedding_kernel(const int64_t* __restrict__ t, const float* __restrict__ freqs, float* __restrict__ out, int B, int dim) {
  const int half = dim / 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * dim) return;
  const int b = i / dim, c = i - b * dim;
  float v = 0.f;
  if (c < 2 * half) {
    const int k = c < half ? c : c - half;
    const float arg = (float)t[b] * freqs[k];
    v = c < half ? cosf(arg) : sinf(arg);
  }
  out[i] = v;
}
extern "C" int pd_timestep_embedding(const int64_t* t, const float* freqs, float* out, int B, int dim, pd_stream_t stream) {
  PD_CHECK_ARG(t && freqs && out && B > 0 && dim > 0, "pd_timestep_embedding: bad args");
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((B * dim + 255) / 256), dim3(256), 0, (hipStream_t)stream, t, freqs, out, B, dim);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- small dense layer (M <= 64 rows): one wave per (row, output column), fp32, float4 loads ----
__global__ void __launch_bounds__(256) linear_small_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ out, int M, int K, int N,
                                                           int act_in, int act_out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int m = blockIdx.y;
  if (n >= N) return;
  const float* w = W + (int64_t)n * K;
  const float* xr = x + (int64_t)m * K;
  float a = 0.f;
  if ((K & 3) == 0) {
    for (int k = lane * 4; k < K; k += 256) {
      const float4 xv = *(const float4*)(xr + k), wv = *(const float4*)(w + k);
      a += act_apply(xv.x, act_in) * wv.x + act_apply(xv.y, act_in) * wv.y + act_apply(xv.z, act_in) * wv.z + act_apply(xv.w, act_in) * wv.w;
    }
  } else {
    for (int k = lane; k < K; k += 64) a += act_apply(xr[k], act_in) * w[k];
  }
  a = wave_sum(a);
  if (lane == 0) out[(int64_t)m * N + n] = act_apply(a + (bias ? bias[n] : 0.f), act_out);
}
extern "C" int pd_linear_small(const float* x, const float* W, const float* b, float* out, int M, int K, int N, int act_in, int act_out,
                               pd_stream_t stream) {
  PD_CHECK_ARG(x && W && out && M > 0 && M <= 65535 && K > 0 && N > 0, "pd_linear_small: bad args (M=%d)", M);
  hipLaunchKernelGGL(linear_small_kernel, dim3((N + 3) / 4, M), dim3(256), 0, (hipStream_t)stream, x, W, b, out, M, K, N, act_in, act_out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- the timestep-embedding chain in four launches instead of seven (pd_time_embed): sinusoid | Linear + SiLU | Linear | every
// per-block SiLU -> Linear projection.  linear_small_kernel gives a wave ONE (row, column): at 32 rows a weight row is fetched 32 times
// and an activation row once per column (268 MB through L2 for the 1024 x 1024 layer), and the input activation is evaluated once per
// column.  Here a workgroup of eight waves owns eight output columns of one layer for ALL rows: a wave keeps its weight row in registers
// (K <= 1024: four float4 per lane), and the activation rows pass through LDS in chunks of 32 rows x 256 columns -- staged once per
// workgroup, the input activation applied on the way in.  The global loads of all four chunks of a row batch are issued together, in
// front of the first one's use: the kernel is a chain of memory latencies (128 workgroups, a few KB each), and this makes it one.
// Per (row, column) a lane adds the same products in the same order as linear_small_kernel (k = 4 lane + 256 i, i ascending, the four
// products of a float4 as contracted there), then the same wave reduction, bias and activation: the outputs are bit-equal to the chain's.
struct te_job {
  const float* W;
  const float* b;
  float* out;
  int N, wg0;                                  // output columns; first workgroup of the job (eight columns per workgroup)
};
struct te_args {
  const float* x;                              // (M, K) rows
  int M, K, njobs;
  te_job job[PD_TIME_EMBED_MAX_PROJ];
};
// ACT_IN / ACT_OUT: PD_ACT_NONE or PD_ACT_SILU, compile-time: the kernel is straight-line code with 96 activation sites, and
// act_apply's run-time switch at each of them made it 11 000 instructions (88 KB: its time was instruction fetch)
template <int ACT_IN, int ACT_OUT>
__global__ void __launch_bounds__(512) linear_rows_kernel(const te_args p) {
  constexpr int MB = 32, KC = 256, NQ = MB * (KC / 4) / 512;   // rows, columns of a staged chunk (32 KB); float4 per thread and chunk
  __shared__ float4 sx[MB * (KC / 4)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int j = 0;
  for (int q = 1; q < p.njobs; ++q)
    if ((int)blockIdx.x >= p.job[q].wg0) j = q;
  const int N = p.job[j].N, K = p.K, M = p.M;
  const int n = ((int)blockIdx.x - p.job[j].wg0) * 8 + wave;
  const bool valid = n < N;                    // (a wave past the last column still stages its share of every chunk)
  const float* __restrict__ w = p.job[j].W + (int64_t)(valid ? n : 0) * K;
  float* __restrict__ out = p.job[j].out;
  const float* __restrict__ x = p.x;
  constexpr int act_in = ACT_IN, act_out = ACT_OUT;
  float4 wv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = lane * 4 + KC * i;
    wv[i] = k < K ? *(const float4*)(w + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float bn = (valid && p.job[j].b) ? p.job[j].b[n] : 0.f;
  for (int m0 = 0; m0 < M; m0 += MB) {
    float4 xs[4][NQ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int idx = tid + 512 * q, m = m0 + idx / (KC / 4), k = KC * i + (idx % (KC / 4)) * 4;
        xs[i][q] = (m < M && k < K) ? *(const float4*)(x + (int64_t)m * K + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    float acc[MB];
#pragma unroll
    for (int r = 0; r < MB; ++r) acc[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (KC * i >= K) break;
      __syncthreads();                         // the previous chunk has been read
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const float4 v = xs[i][q];
        sx[tid + 512 * q] = make_float4(act_apply(v.x, act_in), act_apply(v.y, act_in), act_apply(v.z, act_in), act_apply(v.w, act_in));
      }
      __syncthreads();
      if (lane * 4 + KC * i < K) {             // (the lanes linear_small_kernel's loop runs for this i)
        const float4 wq = wv[i];
#pragma unroll
        for (int r = 0; r < MB; ++r) {
          const float4 xq = sx[r * (KC / 4) + lane];
          // linear_small_kernel's  a += x0 w0 + x1 w1 + x2 w2 + x3 w3  as the compiler contracts it there (one rounded product, three
          // fused ones, one add), spelled out so that the bits do not depend on how this loop is compiled
          float t = xq.y * wq.y;
          t = __builtin_fmaf(xq.x, wq.x, t);
          t = __builtin_fmaf(xq.z, wq.z, t);
          t = __builtin_fmaf(xq.w, wq.w, t);
          acc[r] += t;
        }
      }
    }
    // wave_sum of every row, level by level: per row the adds of wave_sum in its order, the 32 rows' cross-lane moves of a level in
    // flight together (row after row they are 192 dependent LDS round trips: most of the kernel's time)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float u[MB];
#pragma unroll
      for (int r = 0; r < MB; ++r) u[r] = __shfl_xor(acc[r], o, 64);
#pragma unroll
      for (int r = 0; r < MB; ++r) acc[r] += u[r];
    }
    if (lane == 0 && valid) {
#pragma unroll
      for (int r = 0; r < MB; ++r)
        if (m0 + r < M) out[(int64_t)(m0 + r) * N + n] = act_apply(acc[r] + bn, act_out);
    }
  }
}

extern "C" int pd_time_embed_supported(int dim, int E) { return dim > 0 && dim <= 256 && (dim & 3) == 0 && E > 0 && E <= 1024 && (E & 3) == 0; }

extern "C" int pd_time_embed(const int64_t* t, const float* freqs, const float* W0, const float* b0, const float* W2, const float* b2,
                             const float* const* proj_W, const float* const* proj_b, float* const* proj_out, const int* proj_N, int nproj,
                             float* sin_out, float* h1, float* temb, int B, int dim, int E, pd_stream_t stream) {
  PD_CHECK_ARG(t && freqs && W0 && W2 && sin_out && h1 && temb && B > 0, "pd_time_embed: null pointer / bad B (%d)", B);
  PD_CHECK_ARG(pd_time_embed_supported(dim, E), "pd_time_embed: dim (%d) must be a multiple of 4 up to 256, E (%d) one up to 1024", dim, E);
  PD_CHECK_ARG(nproj >= 0 && nproj <= PD_TIME_EMBED_MAX_PROJ && (nproj == 0 || (proj_W && proj_b && proj_out && proj_N)),
               "pd_time_embed: at most %d projections (%d)", PD_TIME_EMBED_MAX_PROJ, nproj);
  const uintptr_t al = (uintptr_t)freqs | (uintptr_t)W0 | (uintptr_t)W2 | (uintptr_t)sin_out | (uintptr_t)h1 | (uintptr_t)temb;
  PD_CHECK_ARG((al & 15) == 0, "pd_time_embed: operands must be 16 B aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((B * dim + 255) / 256), dim3(256), 0, s, t, freqs, sin_out, B, dim);
  PD_CHECK_LAUNCH();
  te_args a = {};
  a.x = sin_out; a.M = B; a.K = dim; a.njobs = 1;
  a.job[0] = te_job{W0, b0, h1, E, 0};
  hipLaunchKernelGGL((linear_rows_kernel<PD_ACT_NONE, PD_ACT_SILU>), dim3((E + 7) / 8), dim3(512), 0, s, a);
  PD_CHECK_LAUNCH();
  a.x = h1; a.K = E;
  a.job[0] = te_job{W2, b2, temb, E, 0};
  hipLaunchKernelGGL((linear_rows_kernel<PD_ACT_NONE, PD_ACT_NONE>), dim3((E + 7) / 8), dim3(512), 0, s, a);
  PD_CHECK_LAUNCH();
  if (nproj == 0) return PD_OK;
  a.x = temb; a.njobs = nproj;
  int wg = 0;
  for (int q = 0; q < nproj; ++q) {
    PD_CHECK_ARG(proj_W[q] && proj_out[q] && proj_N[q] > 0 && ((uintptr_t)proj_W[q] & 15) == 0, "pd_time_embed: projection %d: bad operand", q);
    a.job[q] = te_job{proj_W[q], proj_b[q], proj_out[q], proj_N[q], wg};
    wg += (proj_N[q] + 7) / 8;
  }
  hipLaunchKernelGGL((linear_rows_kernel<PD_ACT_SILU, PD_ACT_NONE>), dim3(wg), dim3(512), 0, s, a);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- x[b, s, :] += table[s, :] ----
__global__ void __launch_bounds__(256) add_rowtable_kernel(float* __restrict__ x, const float* __restrict__ table, int64_t total, int64_t per) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) x[i] += table[i % per];
}
extern "C" int pd_add_rowtable(float* x, const float* table, int64_t n_samples, int rows_per_sample, int C, pd_stream_t stream) {
  PD_CHECK_ARG(x && table, "pd_add_rowtable: null");
  const int64_t per = (int64_t)rows_per_sample * C, total = per * n_samples;
  hipLaunchKernelGGL(add_rowtable_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, table, total, per);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

__global__ void __launch_bounds__(256) add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = a[i] + b[i];
}
extern "C" int pd_add(const float* a, const float* b, float* out, int64_t n, pd_stream_t stream) {
  PD_CHECK_ARG(a && b && out, "pd_add: null");
  hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, a, b, out, n);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- DDPM ancestral step (latent_diffusion.py:553-566, 592-596, 620-631) ----
__global__ void __launch_bounds__(256) ddpm_step_kernel(const float* __restrict__ zt, const float* __restrict__ eps,
                                                        const float* __restrict__ noise, const float* __restrict__ shift,
                                                        const int64_t* __restrict__ t, const float* __restrict__ coef, int T,
                                                        float* __restrict__ out, int64_t per, float temperature, int clip) {
  const int b = blockIdx.y;
  const int tt = (int)t[b];
  const float c_recip = coef[tt], c_recipm1 = coef[T + tt], c1 = coef[2 * T + tt], c2 = coef[3 * T + tt];
  const float sigma = expf(0.5f * coef[4 * T + tt]);
  const float nz = tt != 0 ? 1.f : 0.f;
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float z = zt[base + i];
    float z0 = c_recip * z - c_recipm1 * eps[base + i];
    if (clip) z0 = fminf(1.f, fmaxf(-1.f, z0));
    float mean = c1 * z0 + c2 * z;
    if (shift) mean = mean - sigma * shift[base + i];
    out[base + i] = mean + nz * sigma * (noise[base + i] * temperature);
  }
}
extern "C" int pd_ddpm_step(const float* zt, const float* eps, const float* noise, const float* mean_shift, const int64_t* t,
                            const float* coef, int T, float* out, int B, int64_t per_sample, float temperature, int clip_denoised,
                            pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && noise && t && coef && out && B > 0, "pd_ddpm_step: bad args");
  hipLaunchKernelGGL(ddpm_step_kernel, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise, mean_shift, t, coef,
                     T, out, per_sample, temperature, clip_denoised);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- the fast samplers' step: DDIM, DPM-Solver++(2M) and its SDE form, each plain, guided and held ----
// One body, nine instantiations: what the forms share they share as source, so a held step under mask 0, a guided step with a zero
// shift and the SDE step at c_n = 0 give the plainer form's bits by construction.  Contraction is off and every fused operation is a
// spelled fmaf: the compiler chooses none of the roundings.  (DDIM is parity-unpinned; see the header.  2M and 2M-SDE have no reference
// implementation: schedule.make_dpmpp_2m_coefficients, schedule.make_dpmpp_2m_sde_coefficients.)
//
// SOLVER  row (one per sample)            v, the step's own result
//   0     a_t, a_prev, sigma              sqrt(a_prev) z0 + dir eps + sigma noise    a null `noise` adds 0.f (eta = 0)
//   1     a_t, c_x, c_d, w                c_x z + c_d D,  D = z0 + w (z0 - hist)
//   2     a_t, c_x, c_d, w, c_n           ... + c_n noise
// then gamma where GUIDED, or (gamma, k_x, k_n) where HELD.  z0 = (z - sqrt(1 - a_t) eps) / sqrt(a_t).
//
// `hist` holds the previous step's x0 and is overwritten in place with this step's (every element is read, then written, by the one
// thread that owns it).  w, c_n and k_n are per sample, so the tests on them are wave-uniform.  With w == 0 (the first step, the
// lower-order final step) hist is NOT read: a captured graph's history buffer holds stale or uninitialised data there, and 0 * NaN must
// not reach the output.  With c_n == 0 (eta = 0) the step noise is NOT read, with k_n == 0 (the last step) the hold noise is not.
// Guidance is the step's last operation, v - gamma shift: compile time in the un-held forms, the test of a pointer in the held ones, whose
// rows always carry gamma.  The hold follows it: held = k_x x0 + k_n hnoise  and  out = m == 0 ? v : m == 1 ? held : m held + (1 - m) v.
// The two end points of the mask are selects: a NaN in x0 / hnoise under m == 0, or in v under m == 1, stays where it is.
struct step_operands {         // operands a form does not have are null
  const float *__restrict__ zt, *__restrict__ eps, *__restrict__ noise, *__restrict__ shift, *__restrict__ x0, *__restrict__ mask,
      *__restrict__ hnoise, *__restrict__ coef;
  float *__restrict__ hist, *__restrict__ out;
  int64_t per;
};

__device__ __forceinline__ float hold_select(float v, float m, float x0, const float* hnoise, int64_t j, float k_x, float k_n) {
#pragma clang fp contract(off)
  float held = k_x * x0;
  if (k_n != 0.f) held = fmaf(k_n, hnoise[j], held);
  const float mix = fmaf(m, held, (1.f - m) * v);
  return m == 0.f ? v : m == 1.f ? held : mix;
}

template <int SOLVER, bool GUIDED, bool HELD>
__global__ void __launch_bounds__(256) step_kernel(const step_operands p) {
#pragma clang fp contract(off)
  static_assert(SOLVER >= 0 && SOLVER <= 2 && !(GUIDED && HELD), "three solvers; a held form takes its guidance at run time");
  constexpr int W = SOLVER + 3, NC = W + (HELD ? 3 : GUIDED ? 1 : 0);
  const unsigned b = blockIdx.y;
  const float* row = p.coef + b * NC;
  const float a_t = row[0];
  const float a_prev = row[1], sigma = row[2];                  // columns 1 and 2 by DDIM's names ...
  const float c_x = row[1], c_d = row[2];                       // ... and by 2M's; each solver uses its own
  const float w = SOLVER >= 1 ? row[3] : 0.f, c_n = SOLVER == 2 ? row[4] : 0.f;
  const float gamma = GUIDED || HELD ? row[W] : 0.f, k_x = HELD ? row[W + 1] : 0.f, k_n = HELD ? row[W + 2] : 0.f;
  const float dir = sqrtf(fmaxf(0.f, fmaf(-sigma, sigma, 1.f - a_prev))), sp = sqrtf(a_prev);      // DDIM only
  const float s1 = sqrtf(1.f - a_t), r = 1.f / sqrtf(a_t);
  const int64_t base = (int64_t)b * p.per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.per; i += (int64_t)gridDim.x * 256) {
    const int64_t j = base + i;
    const float z = p.zt[j], e = p.eps[j];
    const float z0 = fmaf(-s1, e, z) * r;
    float v;
    if constexpr (SOLVER == 0) {
      v = fmaf(dir, e, sp * z0) + (p.noise ? sigma * p.noise[j] : 0.f);
    } else {
      float d = z0;
      if (w != 0.f) d = fmaf(w, z0 - p.hist[j], z0);
      v = fmaf(c_d, d, c_x * z);
      if (SOLVER == 2 && c_n != 0.f) v = fmaf(c_n, p.noise[j], v);
    }
    if (HELD ? p.shift != nullptr : GUIDED) v = fmaf(-gamma, p.shift[j], v);
    if constexpr (HELD) v = hold_select(v, p.mask[j], p.x0[j], p.hnoise, j, k_x, k_n);
    p.out[j] = v;
    if constexpr (SOLVER != 0) p.hist[j] = z0;
  }
}

// The launcher behind the nine entry points.  `noise` may be null for DDIM only, `shift` for a held form only.
template <int SOLVER, bool GUIDED, bool HELD>
static int launch_step(const char* fn, const step_operands& p, int B, pd_stream_t stream) {
  PD_CHECK_ARG(p.zt && p.eps && p.coef && p.out && (SOLVER != 2 || p.noise) && (SOLVER == 0 || p.hist) && (!GUIDED || p.shift) && B > 0 &&
                   B <= 65535 && p.per > 0,
               "%s: bad args", fn);
  PD_CHECK_ARG(!HELD || (p.x0 && p.mask && p.hnoise),
               "%s: hold_x0 / hold_mask / hold_noise must not be null (hold_noise is not read where k_n == 0)", fn);
  hipLaunchKernelGGL((step_kernel<SOLVER, GUIDED, HELD>), dim3(grid_for(p.per), B), dim3(256), 0, (hipStream_t)stream, p);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// step_operands in its order: zt, eps, noise, shift, x0, mask, hnoise, coef, hist, out, per
#define NIL nullptr
extern "C" int pd_ddim_step(const float* zt, const float* eps, const float* noise, const float* coef, float* out, int B,
                            int64_t per_sample, pd_stream_t stream) {
  return launch_step<0, false, false>("pd_ddim_step", {zt, eps, noise, NIL, NIL, NIL, NIL, coef, NIL, out, per_sample}, B, stream);
}
extern "C" int pd_ddim_step_guided(const float* zt, const float* eps, const float* noise, const float* shift, const float* coef4, float* out,
                                   int B, int64_t per_sample, pd_stream_t stream) {
  return launch_step<0, true, false>("pd_ddim_step_guided", {zt, eps, noise, shift, NIL, NIL, NIL, coef4, NIL, out, per_sample}, B, stream);
}
extern "C" int pd_ddim_step_held(const float* zt, const float* eps, const float* noise, const float* shift, const float* hold_x0,
                                 const float* hold_mask, const float* hold_noise, const float* coef6, float* out, int B, int64_t per_sample,
                                 pd_stream_t stream) {
  return launch_step<0, false, true>("pd_ddim_step_held", {zt, eps, noise, shift, hold_x0, hold_mask, hold_noise, coef6, NIL, out, per_sample},
                                     B, stream);
}
extern "C" int pd_dpmpp_2m_step(const float* zt, const float* eps, float* hist, const float* coef4, float* out, int B, int64_t per_sample,
                                pd_stream_t stream) {
  return launch_step<1, false, false>("pd_dpmpp_2m_step", {zt, eps, NIL, NIL, NIL, NIL, NIL, coef4, hist, out, per_sample}, B, stream);
}
extern "C" int pd_dpmpp_2m_step_guided(const float* zt, const float* eps, float* hist, const float* shift, const float* coef5, float* out,
                                       int B, int64_t per_sample, pd_stream_t stream) {
  return launch_step<1, true, false>("pd_dpmpp_2m_step_guided", {zt, eps, NIL, shift, NIL, NIL, NIL, coef5, hist, out, per_sample}, B, stream);
}
extern "C" int pd_dpmpp_2m_step_held(const float* zt, const float* eps, float* hist, const float* shift, const float* hold_x0,
                                     const float* hold_mask, const float* hold_noise, const float* coef7, float* out, int B,
                                     int64_t per_sample, pd_stream_t stream) {
  return launch_step<1, false, true>("pd_dpmpp_2m_step_held", {zt, eps, NIL, shift, hold_x0, hold_mask, hold_noise, coef7, hist, out, per_sample},
                                     B, stream);
}
extern "C" int pd_dpmpp_2m_sde_step(const float* zt, const float* eps, const float* noise, float* hist, const float* coef5, float* out, int B,
                                    int64_t per_sample, pd_stream_t stream) {
  return launch_step<2, false, false>("pd_dpmpp_2m_sde_step", {zt, eps, noise, NIL, NIL, NIL, NIL, coef5, hist, out, per_sample}, B, stream);
}
extern "C" int pd_dpmpp_2m_sde_step_guided(const float* zt, const float* eps, const float* noise, float* hist, const float* shift,
                                           const float* coef6, float* out, int B, int64_t per_sample, pd_stream_t stream) {
  return launch_step<2, true, false>("pd_dpmpp_2m_sde_step_guided", {zt, eps, noise, shift, NIL, NIL, NIL, coef6, hist, out, per_sample}, B,
                                     stream);
}
extern "C" int pd_dpmpp_2m_sde_step_held(const float* zt, const float* eps, const float* noise, float* hist, const float* shift,
                                         const float* hold_x0, const float* hold_mask, const float* hold_noise, const float* coef8, float* out,
                                         int B, int64_t per_sample, pd_stream_t stream) {
  return launch_step<2, false, true>("pd_dpmpp_2m_sde_step_held",
                                     {zt, eps, noise, shift, hold_x0, hold_mask, hold_noise, coef8, hist, out, per_sample}, B, stream);
}
#undef NIL

// the start rule: out = hold_select(z, ...) with rows (k_x, k_n) = (sqrt(a_0), sqrt(1 - a_0)).  Every element is read, then written, by
// the one thread that owns it (no __restrict__ on z / noise / out): out may alias z, and noise may be z itself.
__global__ void __launch_bounds__(256) hold_blend_kernel(const float* z, const float* __restrict__ x0, const float* __restrict__ mask,
                                                         const float* noise, const float* __restrict__ coef, float* out, int64_t per) {
  const int b = blockIdx.y;
  const float k_x = coef[b * 2], k_n = coef[b * 2 + 1];
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256)
    out[base + i] = hold_select(z[base + i], mask[base + i], x0[base + i], noise, base + i, k_x, k_n);
}
extern "C" int pd_hold_blend(const float* z, const float* x0, const float* mask, const float* noise, const float* coef2, float* out, int B,
                             int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(z && x0 && mask && noise && coef2 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_hold_blend: bad args");
  hipLaunchKernelGGL(hold_blend_kernel, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, z, x0, mask, noise, coef2, out,
                     per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- NCHW <-> NHWC (fp32) ----
__global__ void __launch_bounds__(256) nchw_to_nhwc_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int C, int HW, int ld) {
  const int64_t total = (int64_t)N * HW * ld;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % ld);
    const int64_t ns = i / ld;
    const int s = (int)(ns % HW);
    const int64_t n = ns / HW;
    out[i] = c < C ? x[(n * C + c) * HW + s] : 0.f;
  }
}
__global__ void __launch_bounds__(256) nhwc_to_nchw_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int C, int HW, int ld) {
  const int64_t total = (int64_t)N * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int s = (int)(i % HW);
    const int64_t nc = i / HW;
    const int c = (int)(nc % C);
    const int64_t n = nc / C;
    out[i] = x[(n * HW + s) * ld + c];
  }
}
extern "C" int pd_nchw_to_nhwc(const float* x, float* out, int N, int C, int HW, int ld_out, pd_stream_t stream) {
  PD_CHECK_ARG(x && out && ld_out >= C, "pd_nchw_to_nhwc: bad args");
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(grid_for((int64_t)N * HW * ld_out)), dim3(256), 0, (hipStream_t)stream, x, out, N, C, HW, ld_out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
extern "C" int pd_nhwc_to_nchw(const float* x, float* out, int N, int C, int HW, int ld_in, pd_stream_t stream) {
  PD_CHECK_ARG(x && out && ld_in >= C, "pd_nhwc_to_nchw: bad args");
  hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(grid_for((int64_t)N * C * HW)), dim3(256), 0, (hipStream_t)stream, x, out, N, C, HW, ld_in);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
