// Fréchet video distance on the device: what the I3D feature engine (prediff_amd/i3d.py) and FrechetVideoDistance (prediff_amd/fvd.py)
// need beside pd_igemm.
//
//   pd_i3d_preprocess          I3DWrapper.preprocess (evaluation/fvd/torchmetrics_wrap.py:33-65) + the channel / time handling of
//                              FrechetVideoDistance.update (:223-233) in one launch, written as the stem convolution's A operand
//   pd_maxpool3d_same          MaxPool3dSamePadding (evaluation/fvd/pytorch_i3d.py:8-35): zero padding that TAKES PART in the max
//   pd_i3d_head                AvgPool3d((2,7,7), 1) -> logits 1x1x1 convolution -> mean over time (pytorch_i3d.py:301-306)
//   pd_feature_moments_update  sum += sum_k f_k, cov_sum += F^T F in fp64 (torchmetrics_wrap.py:241-247), fixed order
//
// The stem (7x7x7, stride 2, 3 input channels) would waste 61 of 64 K columns per filter tap as a plain implicit GEMM, so the preprocess
// kernel writes the im2col along W: row (n, t, y, ow) of the operand holds channel 3 dw + c = frame[y][2 ow - 2 + dw][c] for dw = 0..6 (zero
// outside the frame and in columns 21..63), and the stem runs as a KT = 7, KH = 7, KW = 1 launch with stride (2, 2, 1): K = 49 x 64.
#include "common.h"

namespace PD_NS {

constexpr int I3D_RES = 224;       // side of the centre crop
constexpr int I3D_WO = 112;        // stem output width = operand rows per image row
constexpr int I3D_PW = 2;          // front pad of the stem along W (SAME rule: 224 % 2 == 0 -> pad 7 - 2 = 5, front 5 / 2)

struct pre_geom {
  int64_t N, T, H, W, C;           // input sizes (T before the doubling)
  int64_t sN, sT, sH, sW, sC;      // element strides
  int T2;                          // frames written per video (2 T with auto_t)
  int auto_t;
  int off_h, off_w;                // crop offsets in the resized frame
  float scale_h, scale_w;          // input size / resized size (torch's area_pixel scale at align_corners = False)
  float mul;                       // 1/255 with normalize, else 1
  float post_mul, post_add;        // (2, -1): [0, 1] -> [-1, 1]; (1, 0): frames that are preprocessed already
};

// source index pair and weight of bilinear interpolation, align_corners = False (ATen area_pixel_compute_source_index + guard_index_and_lambda)
__device__ __forceinline__ void bilin_src(int dst, float scale, int in_size, int& i0, int& i1, float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = min((int)s, in_size - 1);
  i1 = min(i0 + 1, in_size - 1);
  l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
}

__global__ void __launch_bounds__(256) i3d_preprocess_kernel(const float* __restrict__ x, const pre_geom g, pd_bf16* __restrict__ out,
                                                             pd_bf16* __restrict__ out_lo, float* __restrict__ out_f32) {
  const int64_t total = g.N * g.T2 * (int64_t)I3D_RES * I3D_WO;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int ow = (int)(idx % I3D_WO);
  const int64_t r1 = idx / I3D_WO;
  const int y = (int)(r1 % I3D_RES);
  const int64_t r2 = r1 / I3D_RES;
  const int t2 = (int)(r2 % g.T2);
  const int64_t n = r2 / g.T2;
  const int ts = g.auto_t ? t2 >> 1 : t2;
  int iy0, iy1;
  float ly;
  bilin_src(y + g.off_h, g.scale_h, (int)g.H, iy0, iy1, ly);
  const float* base = x + n * g.sN + ts * g.sT;
  const float* row0 = base + iy0 * g.sH;
  const float* row1 = base + iy1 * g.sH;
  const int nc = g.C == 1 ? 1 : 3;
  float v[21];
#pragma unroll
  for (int dw = 0; dw < 7; ++dw) {
    const int xw = 2 * ow - I3D_PW + dw;
    const bool ok = xw >= 0 && xw < I3D_RES;
    int ix0, ix1;
    float lx;
    bilin_src(ok ? xw + g.off_w : 0, g.scale_w, (int)g.W, ix0, ix1, lx);
    float last = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c < nc) {
        const int64_t co = c * g.sC;
        const float v00 = row0[ix0 * g.sW + co] * g.mul, v01 = row0[ix1 * g.sW + co] * g.mul;
        const float v10 = row1[ix0 * g.sW + co] * g.mul, v11 = row1[ix1 * g.sW + co] * g.mul;
        const float top = (1.f - lx) * v00 + lx * v01;
        const float bot = (1.f - lx) * v10 + lx * v11;
        last = g.post_mul * ((1.f - ly) * top + ly * bot) + g.post_add;
      }
      v[3 * dw + c] = ok ? last : 0.f;          // one input channel: read as three equal ones
    }
  }
  if (out_f32) {                                 // dw = 2, 3 are pixels 2 ow and 2 ow + 1: the frame itself, channels last
    float* o = out_f32 + ((int64_t)r1 * I3D_RES + 2 * ow) * 3;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = v[6 + k];
  }
  uint32_t hi[32], lo[32];
#pragma unroll
  for (int e = 0; e < 32; ++e) {
    const float a = 2 * e < 21 ? v[2 * e < 21 ? 2 * e : 0] : 0.f;
    const float b = 2 * e + 1 < 21 ? v[2 * e + 1 < 21 ? 2 * e + 1 : 0] : 0.f;
    if (out_lo) {
      uint16_t h0, l0, h1, l1;
      f2bf_split(a, h0, l0);
      f2bf_split(b, h1, l1);
      hi[e] = h0 | ((uint32_t)h1 << 16);
      lo[e] = l0 | ((uint32_t)l1 << 16);
    } else {
      hi[e] = (uint32_t)f2op(a) | ((uint32_t)f2op(b) << 16);
      lo[e] = 0;
    }
  }
  uint4* o = (uint4*)(out + idx * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = make_uint4(hi[4 * q], hi[4 * q + 1], hi[4 * q + 2], hi[4 * q + 3]);
  if (out_lo) {
    uint4* ol = (uint4*)(out_lo + idx * 64);
#pragma unroll
    for (int q = 0; q < 8; ++q) ol[q] = make_uint4(lo[4 * q], lo[4 * q + 1], lo[4 * q + 2], lo[4 * q + 3]);
  }
}

#if !PD_IS_F16
extern "C" int pd_f16_i3d_preprocess(const float*, const int64_t*, const int64_t*, int, int, int, pd_bf16*, pd_bf16*, float*, const pd_call_opts*,
                                     pd_stream_t);
extern "C" int pd_f16_maxpool3d_same(const float*, float*, pd_bf16*, pd_bf16*, int, int, int, int, int, int, int, int, int, int, int, int, int,
                                     int, const pd_call_opts*, pd_stream_t);
#endif

extern "C" int PD_ENTRY(i3d_preprocess)(const float* x, const int64_t* sizes, const int64_t* strides, int normalize, int auto_t, int rescale,
                                        pd_bf16* out, pd_bf16* out_lo, float* out_f32, const pd_call_opts* opts, pd_stream_t stream) {
  PD_FORWARD_F16(PD_OPTS_F16(opts), pd_f16_i3d_preprocess(x, sizes, strides, normalize, auto_t, rescale, out, out_lo, out_f32, opts, stream));
  PD_CHECK_ARG(!PD_IS_F16 || !out_lo, "pd_i3d_preprocess: the hi/lo split exists for bfloat16 operands only");
  PD_CHECK_ARG(x && sizes && strides && out, "pd_i3d_preprocess: null pointer");
  PD_CHECK_ARG((((uintptr_t)out | (uintptr_t)out_lo) & 15) == 0, "pd_i3d_preprocess: the operand rows must be 16 B aligned");
  pre_geom g;
  g.N = sizes[0]; g.T = sizes[1]; g.H = sizes[2]; g.W = sizes[3]; g.C = sizes[4];
  g.sN = strides[0]; g.sT = strides[1]; g.sH = strides[2]; g.sW = strides[3]; g.sC = strides[4];
  PD_CHECK_ARG(g.N > 0 && g.T > 0 && g.H > 0 && g.W > 0 && g.H < (1 << 20) && g.W < (1 << 20), "pd_i3d_preprocess: bad sizes");
  PD_CHECK_ARG(g.C == 1 || g.C == 3, "pd_i3d_preprocess: %lld channels (1 or 3 are supported)", (long long)g.C);
  g.auto_t = auto_t ? 1 : 0;
  PD_CHECK_ARG(g.T * (g.auto_t + 1) < (1 << 20), "pd_i3d_preprocess: too many frames");
  g.T2 = (int)(g.T * (g.auto_t + 1));
  // the short side goes to 224, the other one to ceil(side * 224 / short side) -- in double, as the reference's Python does
  const double scale = (double)I3D_RES / (double)(g.H < g.W ? g.H : g.W);
  int64_t RH, RW;
  if (g.H < g.W) { RH = I3D_RES; RW = (int64_t)ceil((double)g.W * scale); }
  else { RH = (int64_t)ceil((double)g.H * scale); RW = I3D_RES; }
  PD_CHECK_ARG(RH >= I3D_RES && RW >= I3D_RES && RH < (1 << 24) && RW < (1 << 24), "pd_i3d_preprocess: bad resize target");
  g.off_h = (int)((RH - I3D_RES) / 2);
  g.off_w = (int)((RW - I3D_RES) / 2);
  g.scale_h = (float)g.H / (float)RH;
  g.scale_w = (float)g.W / (float)RW;
  g.mul = normalize ? 1.0f / 255.0f : 1.0f;
  g.post_mul = rescale ? 2.0f : 1.0f;
  g.post_add = rescale ? -1.0f : 0.0f;
  const int64_t total = g.N * g.T2 * (int64_t)I3D_RES * I3D_WO;
  PD_CHECK_ARG((total + 255) / 256 < 0x7fffffffll, "pd_i3d_preprocess: too many rows for one launch");
  hipLaunchKernelGGL(i3d_preprocess_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, g, out, out_lo, out_f32);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------- max-pool
struct pool_geom {
  int B, T, H, W, C, ld_in;
  int To, Ho, Wo;
  int kt, kh, kw, st, sh, sw, pt, ph, pw;      // pt / ph / pw: FRONT pads
  int ld_out, ld_outb;
};

// one thread: four channels of one output position; the window's taps outside the tensor count as the value 0 (the reference pads with
// zeros and then pools)
__global__ void __launch_bounds__(256) maxpool3d_same_kernel(const float* __restrict__ x, const pool_geom g, float* __restrict__ out_f32,
                                                             pd_bf16* __restrict__ outb, pd_bf16* __restrict__ outb_lo) {
  const int c4n = g.C >> 2;
  const int64_t total = (int64_t)g.B * g.To * g.Ho * g.Wo * c4n;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c4n) * 4;
  const int64_t pos = idx / c4n;
  const int ow = (int)(pos % g.Wo);
  const int64_t r1 = pos / g.Wo;
  const int oh = (int)(r1 % g.Ho);
  const int64_t r2 = r1 / g.Ho;
  const int ot = (int)(r2 % g.To);
  const int b = (int)(r2 / g.To);
  const int t0 = ot * g.st - g.pt, h0 = oh * g.sh - g.ph, w0 = ow * g.sw - g.pw;
  const float NEG = -__builtin_inff();
  float4 m = make_float4(NEG, NEG, NEG, NEG);
  bool padded = false;
  for (int a = 0; a < g.kt; ++a) {
    const int t = t0 + a;
    for (int e = 0; e < g.kh; ++e) {
      const int h = h0 + e;
      for (int f = 0; f < g.kw; ++f) {
        const int w = w0 + f;
        if ((unsigned)t < (unsigned)g.T && (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)g.W) {
          const float4 v = *(const float4*)(x + ((((int64_t)b * g.T + t) * g.H + h) * g.W + w) * g.ld_in + c);
          m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w;
        } else {
          padded = true;
        }
      }
    }
  }
  if (padded) { m.x = m.x > 0.f ? m.x : 0.f; m.y = m.y > 0.f ? m.y : 0.f; m.z = m.z > 0.f ? m.z : 0.f; m.w = m.w > 0.f ? m.w : 0.f; }
  if (out_f32) *(float4*)(out_f32 + pos * g.ld_out + c) = m;
  if (outb) {
    uint32_t h01, h23, l01 = 0, l23 = 0;
    if (outb_lo) {
      uint16_t h0_, l0_, h1_, l1_, h2_, l2_, h3_, l3_;
      f2bf_split(m.x, h0_, l0_); f2bf_split(m.y, h1_, l1_); f2bf_split(m.z, h2_, l2_); f2bf_split(m.w, h3_, l3_);
      h01 = h0_ | ((uint32_t)h1_ << 16); h23 = h2_ | ((uint32_t)h3_ << 16);
      l01 = l0_ | ((uint32_t)l1_ << 16); l23 = l2_ | ((uint32_t)l3_ << 16);
      *(uint2*)(outb_lo + pos * g.ld_outb + c) = make_uint2(l01, l23);
    } else {
      h01 = pack_op2(m.x, m.y); h23 = pack_op2(m.z, m.w);
    }
    *(uint2*)(outb + pos * g.ld_outb + c) = make_uint2(h01, h23);
  }
}

static inline int same_pad(int k, int s, int size) {
  const int p = size % s == 0 ? k - s : k - size % s;
  return p > 0 ? p : 0;
}

extern "C" int PD_ENTRY(maxpool3d_same)(const float* x, float* out_f32, pd_bf16* outb, pd_bf16* outb_lo, int B, int T, int H, int W, int C,
                                        int ld_in, int kt, int kh, int kw, int st, int sh, int sw, int ld_out, int ld_outb,
                                        const pd_call_opts* opts, pd_stream_t stream) {
  PD_FORWARD_F16(PD_OPTS_F16(opts), pd_f16_maxpool3d_same(x, out_f32, outb, outb_lo, B, T, H, W, C, ld_in, kt, kh, kw, st, sh, sw, ld_out,
                                                          ld_outb, opts, stream));
  PD_CHECK_ARG(!PD_IS_F16 || !outb_lo, "pd_maxpool3d_same: the hi/lo split exists for bfloat16 operands only");
  PD_CHECK_ARG(x && (out_f32 || outb) && (!outb_lo || outb), "pd_maxpool3d_same: null pointer");
  PD_CHECK_ARG(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && (C & 3) == 0 && ld_in >= C && (ld_in & 3) == 0,
               "pd_maxpool3d_same: bad sizes (C=%d and ld_in=%d must be multiples of 4)", C, ld_in);
  PD_CHECK_ARG(kt > 0 && kh > 0 && kw > 0 && st > 0 && sh > 0 && sw > 0 && kt >= st && kh >= sh && kw >= sw, "pd_maxpool3d_same: bad window");
  PD_CHECK_ARG((!out_f32 || (ld_out >= C && (ld_out & 3) == 0)) && (!outb || (ld_outb >= C && (ld_outb & 3) == 0)),
               "pd_maxpool3d_same: the output rows must hold C columns and be multiples of 4");
  PD_CHECK_ARG((((uintptr_t)x | (uintptr_t)out_f32) & 15) == 0 && (((uintptr_t)outb | (uintptr_t)outb_lo) & 7) == 0,
               "pd_maxpool3d_same: misaligned pointer");
  pool_geom g;
  g.B = B; g.T = T; g.H = H; g.W = W; g.C = C; g.ld_in = ld_in;
  g.kt = kt; g.kh = kh; g.kw = kw; g.st = st; g.sh = sh; g.sw = sw;
  const int pT = same_pad(kt, st, T), pH = same_pad(kh, sh, H), pW = same_pad(kw, sw, W);
  g.pt = pT / 2; g.ph = pH / 2; g.pw = pW / 2;
  g.To = (T + pT - kt) / st + 1; g.Ho = (H + pH - kh) / sh + 1; g.Wo = (W + pW - kw) / sw + 1;
  g.ld_out = ld_out; g.ld_outb = ld_outb;
  const int64_t total = (int64_t)B * g.To * g.Ho * g.Wo * (C >> 2);
  PD_CHECK_ARG((total + 255) / 256 < 0x7fffffffll, "pd_maxpool3d_same: too many outputs for one launch");
  hipLaunchKernelGGL(maxpool3d_same_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, g, out_f32, outb,
                     outb_lo);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

#if !PD_IS_F16
// ------------------------------------------------------------------------------------------------------------------------- head (fp32)
// pooled[b][c] = sum_t wt(t) sum_hw x[b][t][hw][c]: the mean over the T - 1 windows of AvgPool3d((2, HW), stride 1), which commutes with the
// linear layer behind it.  A frame lies in (t >= 1) + (t <= T - 2) windows of 2 HW values each.
__global__ void __launch_bounds__(256) i3d_head_pool_kernel(const float* __restrict__ x, float* __restrict__ pooled, int T, int HW, int C) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (c >= C) return;
  const float* p = x + (int64_t)b * T * HW * C + c;
  const float inv = 1.0f / (2.0f * (float)HW * (float)(T - 1));
  float acc = 0.f;
  for (int t = 0; t < T; ++t) {
    float s = 0.f;
    for (int i = 0; i < HW; ++i) s += p[((int64_t)t * HW + i) * C];
    acc += s * ((float)((t >= 1) + (t <= T - 2)) * inv);
  }
  pooled[(int64_t)b * C + c] = acc;
}

// out[b][n] = W[n] . pooled[b] + bias[n]: one wave per output, lanes stride over K, butterfly sum (a fixed order)
__global__ void __launch_bounds__(256) i3d_head_logits_kernel(const float* __restrict__ pooled, const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ out, int K, int N) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  if (n >= N) return;
  const float* w = W + (int64_t)n * K;
  const float* v = pooled + (int64_t)b * K;
  float acc = 0.f;
  for (int k = lane; k < K; k += 64) acc = fmaf(w[k], v[k], acc);
  acc = wave_sum(acc);
  if (lane == 0) out[(int64_t)b * N + n] = acc + (bias ? bias[n] : 0.f);
}

extern "C" int pd_i3d_head(const float* x, const float* W, const float* bias, float* pooled, float* out, int B, int T, int HW, int C, int N,
                           pd_stream_t stream) {
  PD_CHECK_ARG(x && W && pooled && out, "pd_i3d_head: null pointer");
  PD_CHECK_ARG(B > 0 && B <= 65535 && T >= 2 && HW > 0 && C > 0 && N > 0, "pd_i3d_head: bad sizes (B=%d, T=%d: the (2, 7, 7) pool needs two frames)", B, T);
  hipLaunchKernelGGL(i3d_head_pool_kernel, dim3((C + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, x, pooled, T, HW, C);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(i3d_head_logits_kernel, dim3((N + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, pooled, W, bias, out, C, N);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------- moments
// cov_sum[i][j] += sum_k f[k][i] f[k][j], sum[j] += sum_k f[k][j] in fp64.  One thread owns one (i, j) and walks k upwards: no atomics, the
// same inputs give the same bits; an fp32 x fp32 product is exact in fp64, so the only rounding is that of the n additions.
constexpr int MOM_TILE = 16, MOM_ROWS = 64;
__global__ void __launch_bounds__(256) feature_moments_kernel(const float* __restrict__ f, int n, int d, int ld, double* __restrict__ sum,
                                                              double* __restrict__ cov) {
  __shared__ float sI[MOM_ROWS][MOM_TILE], sJ[MOM_ROWS][MOM_TILE];
  const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
  const int i0 = blockIdx.y * MOM_TILE, j0 = blockIdx.x * MOM_TILE;
  const int i = i0 + ti, j = j0 + tj;
  double acc = 0.0, s = 0.0;
  for (int k0 = 0; k0 < n; k0 += MOM_ROWS) {
    __syncthreads();
    for (int e = threadIdx.x; e < MOM_ROWS * MOM_TILE; e += 256) {
      const int r = e >> 4, c = e & 15, k = k0 + r;
      sI[r][c] = (k < n && i0 + c < d) ? f[(int64_t)k * ld + i0 + c] : 0.f;
      sJ[r][c] = (k < n && j0 + c < d) ? f[(int64_t)k * ld + j0 + c] : 0.f;
    }
    __syncthreads();
    const int rows = min(MOM_ROWS, n - k0);
    for (int r = 0; r < rows; ++r) {
      acc += (double)sI[r][ti] * (double)sJ[r][tj];
      s += (double)sJ[r][tj];
    }
  }
  if (i < d && j < d) cov[(int64_t)i * d + j] += acc;
  if (blockIdx.y == 0 && ti == 0 && j < d) sum[j] += s;
}

extern "C" int pd_feature_moments_update(const float* f, int64_t n, int d, int ld, double* sum, double* cov_sum, pd_stream_t stream) {
  PD_CHECK_ARG(f && sum && cov_sum, "pd_feature_moments_update: null pointer");
  PD_CHECK_ARG(n >= 1 && n < (1ll << 30) && d >= 1 && d <= 4096 && ld >= d, "pd_feature_moments_update: bad sizes (n=%lld, d=%d, ld=%d)",
               (long long)n, d, ld);
  const int tiles = (d + MOM_TILE - 1) / MOM_TILE;
  hipLaunchKernelGGL(feature_moments_kernel, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, f, (int)n, d, ld, sum, cov_sum);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
#endif

}  // namespace PD_NS
