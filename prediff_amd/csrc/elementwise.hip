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

// ---- DDIM step (parity-unpinned; see header) ----
// GUIDED: coefficient rows (a_t, a_prev, sigma, gamma) and the knowledge-alignment shift, subtracted as the very last operation
// (out - gamma * shift), so a zero shift gives the un-guided result bit for bit.  The shift pointer is a trailing parameter pack
// (one pointer when GUIDED, none otherwise): the un-guided instantiation has exactly the kernel arguments, and so the kernel-argument
// offsets and the instruction stream, of the single-mode kernel it replaces.
template <typename P> __device__ __forceinline__ P first_of(P p) { return p; }
template <bool GUIDED, typename... Shift>
__global__ void __launch_bounds__(256) ddim_step_kernel(const float* __restrict__ zt, const float* __restrict__ eps,
                                                        const float* __restrict__ noise, const float* __restrict__ coef,
                                                        float* __restrict__ out, int64_t per, const Shift* __restrict__... shift) {
  static_assert(sizeof...(Shift) == (GUIDED ? 1 : 0), "the guided step takes one shift pointer, the un-guided none");
  constexpr int NC = GUIDED ? 4 : 3;
  const int b = blockIdx.y;
  const float a_t = coef[b * NC], a_prev = coef[b * NC + 1], sigma = coef[b * NC + 2];
  const float s1 = sqrtf(1.f - a_t), r = 1.f / sqrtf(a_t), sp = sqrtf(a_prev);
  const float dir = sqrtf(fmaxf(0.f, 1.f - a_prev - sigma * sigma));
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float e = eps[base + i];
    const float z0 = (zt[base + i] - s1 * e) * r;
    float v = sp * z0 + dir * e + (noise ? sigma * noise[base + i] : 0.f);
    if constexpr (GUIDED) v = v - coef[b * NC + 3] * first_of(shift...)[base + i];
    out[base + i] = v;
  }
}
extern "C" int pd_ddim_step(const float* zt, const float* eps, const float* noise, const float* coef, float* out, int B,
                            int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && coef && out && B > 0, "pd_ddim_step: bad args");
  hipLaunchKernelGGL(ddim_step_kernel<false>, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise, coef, out,
                     per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
extern "C" int pd_ddim_step_guided(const float* zt, const float* eps, const float* noise, const float* shift, const float* coef4, float* out,
                                   int B, int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && shift && coef4 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_ddim_step_guided: bad args");
  hipLaunchKernelGGL((ddim_step_kernel<true, float>), dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise, coef4, out,
                     per_sample, shift);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- DPM-Solver++(2M) step, data prediction (no reference implementation; DESIGN.md §7, schedule.make_dpmpp_2m_coefficients) ----
// Coefficient rows (a_t, c_x, c_d, w[, gamma]) per sample.  `hist` holds the previous step's x0 and is overwritten in place with this
// step's (every element is read, then written, by the one thread that owns it).  w is per sample, so the `w != 0` test is wave-uniform;
// with w == 0 (the first step, the lower-order final step) hist is NOT read: a captured graph's history buffer holds stale or
// uninitialised data there, and 0 * NaN must not reach the output.  GUIDED: as ddim_step_kernel, `- gamma * shift` last.
template <bool GUIDED, typename... Shift>
__global__ void __launch_bounds__(256) dpmpp_2m_step_kernel(const float* __restrict__ zt, const float* __restrict__ eps,
                                                            float* __restrict__ hist, const float* __restrict__ coef,
                                                            float* __restrict__ out, int64_t per, const Shift* __restrict__... shift) {
  static_assert(sizeof...(Shift) == (GUIDED ? 1 : 0), "the guided step takes one shift pointer, the un-guided none");
  constexpr int NC = GUIDED ? 5 : 4;
  const int b = blockIdx.y;
  const float a_t = coef[b * NC], c_x = coef[b * NC + 1], c_d = coef[b * NC + 2], w = coef[b * NC + 3];
  const float s1 = sqrtf(1.f - a_t), r = 1.f / sqrtf(a_t);
  const bool second_order = w != 0.f;
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float z = zt[base + i];
    const float z0 = fmaf(-s1, eps[base + i], z) * r;      // explicit FMAs: both instantiations round alike, whatever the contraction pass picks
    float d = z0;
    if (second_order) d = fmaf(w, z0 - hist[base + i], z0);
    float v = fmaf(c_d, d, c_x * z);
    if constexpr (GUIDED) v = v - coef[b * NC + 4] * first_of(shift...)[base + i];
    out[base + i] = v;
    hist[base + i] = z0;
  }
}
extern "C" int pd_dpmpp_2m_step(const float* zt, const float* eps, float* hist, const float* coef4, float* out, int B, int64_t per_sample,
                                pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && hist && coef4 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_dpmpp_2m_step: bad args");
  hipLaunchKernelGGL(dpmpp_2m_step_kernel<false>, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, hist, coef4, out,
                     per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
extern "C" int pd_dpmpp_2m_step_guided(const float* zt, const float* eps, float* hist, const float* shift, const float* coef5, float* out,
                                       int B, int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && hist && shift && coef5 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_dpmpp_2m_step_guided: bad args");
  hipLaunchKernelGGL((dpmpp_2m_step_kernel<true, float>), dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, hist, coef5,
                     out, per_sample, shift);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- SDE-DPM-Solver++(2M) step (schedule.make_dpmpp_2m_sde_coefficients) ----
// dpmpp_2m_step_kernel with a noise term: rows (a_t, c_x, c_d, w, c_n[, gamma]) per sample, out = c_x z + c_d D + c_n n.  c_n is per
// sample like w, so the `c_n != 0` test is wave-uniform; with c_n == 0 (eta = 0) the noise buffer is NOT read and the operations
// are dpmpp_2m_step_kernel's in its order, so the result is pd_dpmpp_2m_step's bit for bit whatever the buffer holds.
template <bool GUIDED, typename... Shift>
__global__ void __launch_bounds__(256) dpmpp_2m_sde_step_kernel(const float* __restrict__ zt, const float* __restrict__ eps,
                                                                const float* __restrict__ noise, float* __restrict__ hist,
                                                                const float* __restrict__ coef, float* __restrict__ out, int64_t per,
                                                                const Shift* __restrict__... shift) {
  static_assert(sizeof...(Shift) == (GUIDED ? 1 : 0), "the guided step takes one shift pointer, the un-guided none");
  constexpr int NC = GUIDED ? 6 : 5;
  const int b = blockIdx.y;
  const float a_t = coef[b * NC], c_x = coef[b * NC + 1], c_d = coef[b * NC + 2], w = coef[b * NC + 3], c_n = coef[b * NC + 4];
  const float s1 = sqrtf(1.f - a_t), r = 1.f / sqrtf(a_t);
  const bool second_order = w != 0.f, stochastic = c_n != 0.f;
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float z = zt[base + i];
    const float z0 = fmaf(-s1, eps[base + i], z) * r;
    float d = z0;
    if (second_order) d = fmaf(w, z0 - hist[base + i], z0);
    float v = fmaf(c_d, d, c_x * z);
    if (stochastic) v = fmaf(c_n, noise[base + i], v);
    if constexpr (GUIDED) v = v - coef[b * NC + 5] * first_of(shift...)[base + i];
    out[base + i] = v;
    hist[base + i] = z0;
  }
}
extern "C" int pd_dpmpp_2m_sde_step(const float* zt, const float* eps, const float* noise, float* hist, const float* coef5, float* out, int B,
                                    int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && noise && hist && coef5 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_dpmpp_2m_sde_step: bad args");
  hipLaunchKernelGGL(dpmpp_2m_sde_step_kernel<false>, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise, hist,
                     coef5, out, per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
extern "C" int pd_dpmpp_2m_sde_step_guided(const float* zt, const float* eps, const float* noise, float* hist, const float* shift,
                                           const float* coef6, float* out, int B, int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && noise && hist && shift && coef6 && out && B > 0 && B <= 65535 && per_sample > 0,
               "pd_dpmpp_2m_sde_step_guided: bad args");
  hipLaunchKernelGGL((dpmpp_2m_sde_step_kernel<true, float>), dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise,
                     hist, coef6, out, per_sample, shift);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ---- held-region (inpainting) forms of the three step kernels ("Held regions") ----
// The step's own result v, then  held = k_x x0 + k_n hnoise  and  out = m == 0 ? v : m == 1 ? held : m held + (1 - m) v  in the same
// launch.  Rows: the un-held row, gamma (read only with a shift pointer), then (k_x, k_n).  v is spelled with the operations the
// un-held kernels compile to (the products they fuse are explicit FMAs here, and contraction is off, so nothing else is fused): where
// m == 0 the output is theirs bit for bit.  The two end points of the mask are selects: a NaN in x0 / hnoise under m == 0, or in v under
// m == 1, stays where it is.  k_n is per sample like w and c_n: with k_n == 0 (the last step) hnoise is NOT read.
__device__ __forceinline__ float hold_select(float v, float m, float x0, const float* hnoise, int64_t j, float k_x, float k_n) {
#pragma clang fp contract(off)
  float held = k_x * x0;
  if (k_n != 0.f) held = fmaf(k_n, hnoise[j], held);
  const float mix = fmaf(m, held, (1.f - m) * v);
  return m == 0.f ? v : m == 1.f ? held : mix;
}

__global__ void __launch_bounds__(256) ddim_step_held_kernel(const float* __restrict__ zt, const float* __restrict__ eps,
                                                             const float* __restrict__ noise, const float* __restrict__ shift,
                                                             const float* __restrict__ x0, const float* __restrict__ mask,
                                                             const float* __restrict__ hnoise, const float* __restrict__ coef,
                                                             float* __restrict__ out, int64_t per) {
#pragma clang fp contract(off)
  constexpr int NC = 6;                          // a_t, a_prev, sigma, gamma, k_x, k_n
  const int b = blockIdx.y;
  const float a_t = coef[b * NC], a_prev = coef[b * NC + 1], sigma = coef[b * NC + 2], gamma = coef[b * NC + 3];
  const float k_x = coef[b * NC + 4], k_n = coef[b * NC + 5];
  const float s1 = sqrtf(1.f - a_t), r = 1.f / sqrtf(a_t), sp = sqrtf(a_prev);
  const float dir = sqrtf(fmaxf(0.f, fmaf(-sigma, sigma, 1.f - a_prev)));
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float e = eps[base + i];
    const float z0 = fmaf(-s1, e, zt[base + i]) * r;
    float v = fmaf(dir, e, sp * z0) + (noise ? sigma * noise[base + i] : 0.f);
    if (shift) v = fmaf(-gamma, shift[base + i], v);
    out[base + i] = hold_select(v, mask[base + i], x0[base + i], hnoise, base + i, k_x, k_n);
  }
}

// SDE = false: rows (a_t, c_x, c_d, w, gamma, k_x, k_n) and no noise pointer; SDE = true: rows (a_t, c_x, c_d, w, c_n, gamma, k_x, k_n)
template <bool SDE>
__global__ void __launch_bounds__(256) dpmpp_2m_step_held_kernel(const float* __restrict__ zt, const float* __restrict__ eps,
                                                                 const float* __restrict__ noise, float* __restrict__ hist,
                                                                 const float* __restrict__ shift, const float* __restrict__ x0,
                                                                 const float* __restrict__ mask, const float* __restrict__ hnoise,
                                                                 const float* __restrict__ coef, float* __restrict__ out, int64_t per) {
#pragma clang fp contract(off)
  constexpr int NC = SDE ? 8 : 7, G = SDE ? 5 : 4;
  const int b = blockIdx.y;
  const float a_t = coef[b * NC], c_x = coef[b * NC + 1], c_d = coef[b * NC + 2], w = coef[b * NC + 3];
  const float c_n = SDE ? coef[b * NC + 4] : 0.f;
  const float gamma = coef[b * NC + G], k_x = coef[b * NC + G + 1], k_n = coef[b * NC + G + 2];
  const float s1 = sqrtf(1.f - a_t), r = 1.f / sqrtf(a_t);
  const bool second_order = w != 0.f, stochastic = c_n != 0.f;
  const int64_t base = (int64_t)b * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (int64_t)gridDim.x * 256) {
    const float z = zt[base + i];
    const float z0 = fmaf(-s1, eps[base + i], z) * r;
    float d = z0;
    if (second_order) d = fmaf(w, z0 - hist[base + i], z0);
    float v = fmaf(c_d, d, c_x * z);
    if constexpr (SDE) {
      if (stochastic) v = fmaf(c_n, noise[base + i], v);
    }
    if (shift) v = fmaf(-gamma, shift[base + i], v);
    out[base + i] = hold_select(v, mask[base + i], x0[base + i], hnoise, base + i, k_x, k_n);
    hist[base + i] = z0;
  }
}

#define PD_CHECK_HOLD(fn) \
  PD_CHECK_ARG(hold_x0 && hold_mask && hold_noise, fn ": hold_x0 / hold_mask / hold_noise must not be null (hold_noise is not read where k_n == 0)")

extern "C" int pd_ddim_step_held(const float* zt, const float* eps, const float* noise, const float* shift, const float* hold_x0,
                                 const float* hold_mask, const float* hold_noise, const float* coef6, float* out, int B, int64_t per_sample,
                                 pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && coef6 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_ddim_step_held: bad args");
  PD_CHECK_HOLD("pd_ddim_step_held");
  hipLaunchKernelGGL(ddim_step_held_kernel, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise, shift, hold_x0,
                     hold_mask, hold_noise, coef6, out, per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
extern "C" int pd_dpmpp_2m_step_held(const float* zt, const float* eps, float* hist, const float* shift, const float* hold_x0,
                                     const float* hold_mask, const float* hold_noise, const float* coef7, float* out, int B,
                                     int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && hist && coef7 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_dpmpp_2m_step_held: bad args");
  PD_CHECK_HOLD("pd_dpmpp_2m_step_held");
  hipLaunchKernelGGL(dpmpp_2m_step_held_kernel<false>, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps,
                     (const float*)nullptr, hist, shift, hold_x0, hold_mask, hold_noise, coef7, out, per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
extern "C" int pd_dpmpp_2m_sde_step_held(const float* zt, const float* eps, const float* noise, float* hist, const float* shift,
                                         const float* hold_x0, const float* hold_mask, const float* hold_noise, const float* coef8, float* out,
                                         int B, int64_t per_sample, pd_stream_t stream) {
  PD_CHECK_ARG(zt && eps && noise && hist && coef8 && out && B > 0 && B <= 65535 && per_sample > 0, "pd_dpmpp_2m_sde_step_held: bad args");
  PD_CHECK_HOLD("pd_dpmpp_2m_sde_step_held");
  hipLaunchKernelGGL(dpmpp_2m_step_held_kernel<true>, dim3(grid_for(per_sample), B), dim3(256), 0, (hipStream_t)stream, zt, eps, noise, hist,
                     shift, hold_x0, hold_mask, hold_noise, coef8, out, per_sample);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

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
