// Stochastic extrapolation (STEPS; S-PROG without noise; DESIGN.md §7 "Stochastic extrapolation"; prediff_amd/steps.py, whose module
// docstring is the definition and numbers the steps; tests/_steps_ref.py restates it).  fp32 fields, fp64 statistics, no atomics: the same
// input gives the same bits.
//
// Every kernel is one 1024-thread workgroup around one frame.  The transform kernels hold one padded complex frame in LDS (pitch W + 1,
// 132 KiB at 128 x 128, plus the twiddle table: the layout of spectrum_lds_kernel, the FFT core of fft_lds.h); a pixel i = y W + x belongs
// to thread i % 1024 in every pass, so whatever a thread reads back from the workspace it wrote itself.  The inverse transform is the forward
// one on conjugated data, scaled by 1 / (H W).
//
// Packing.  Every filter here (the band weights w_l, the noise filter P) is real and even, so a complex frame carries two real fields
// through filter and inverse transform at once:
//   analyse   A_0 + i A_1 (one forward transform, one inverse per level); with AR(2) A_2 travels alone;
//   evolve    w_l S + i w_(l+1) S with S = P FFT(z) the shaped spectrum of ONE member's white field (Hermitian: z is real), whose inverse
//             is e_l + i e_(l+1): one inverse per PAIR OF LEVELS; an odd number of levels leaves the last pair half empty.
// Members are not packed with each other: the rounding of a complex transform mixes its two fields, and a member alone must give the bits
// it gives inside an ensemble.
//
//   steps_analyse_kernel  one workgroup per sequence: steps 0 .. 5.  Leaves N_l0, N_l1 and P in the workspace.
//   steps_evolve_kernel   one workgroup per (member, sequence), looping over the leads: steps 6 .. 8.  Its level states (two per level) live
//                         in the workspace; lead 1 and 2 read the analysis' N in place.
//   steps_finish_kernel   one workgroup per (member, sequence, lead): step 9, the frame after mask / match / cut in LDS, pd_advect's rule.
// Sums: lane-strided fp64, a fixed-order wave butterfly, the waves' partials added in wave order by every thread (block_sum); block_sum, the
// bilinear rule, the pixel loop and fft2d are in frame_lds.h, which anvil.hip shares.
#include "common.h"
#include "fft_lds.h"
#include "frame_lds.h"

namespace {

constexpr int ST_MAX_MEMBERS = 512;
constexpr double ST_EPS = 1e-6, ST_DEAD = 1e-10;

// mean and population variance of the two fields (re, -im) * inv of the frame in LDS, fp64: mean[2], var[2]
__device__ __forceinline__ void frame_stats(const float2* __restrict__ z, int H, int W, int pitch, float inv, double* __restrict__ red,
                                            double (&mean)[2], double (&var)[2]) {
  const int HW = H * W;
  double s[2] = {0.0, 0.0};
  ST_PIXELS(const float2 c = z[li]; s[0] += (double)(c.x * inv); s[1] += (double)(-c.y * inv);)
  block_sum<2>(s, red);
  mean[0] = s[0] / (double)HW, mean[1] = s[1] / (double)HW;
  double q[2] = {0.0, 0.0};
  ST_PIXELS(const float2 c = z[li]; const double d0 = (double)(c.x * inv) - mean[0], d1 = (double)(-c.y * inv) - mean[1];
            q[0] += d0 * d0; q[1] += d1 * d1;)
  block_sum<2>(q, red);
  var[0] = q[0] / (double)HW, var[1] = q[1] / (double)HW;
}

// grid: B.  dynamic LDS: (H (W + 1) + max(H, W)) complex + ST_RED doubles.
// wsN [B][L][2][HW]: N_l0, N_l1.  wsP [B][HW].  wsZ [B][2][HW] complex: the transforms of A_0 + i A_1 and of A_2.
__global__ void __launch_bounds__(ST_THREADS) steps_analyse_kernel(const float* __restrict__ ctx, const float* __restrict__ motion,
                                                                   const float* __restrict__ bands, int T, int H, int W, int L, int ar,
                                                                   float thr, float* __restrict__ mu, float* __restrict__ sigma,
                                                                   float* __restrict__ phi, float* __restrict__ gamma, float* wsN,
                                                                   float* __restrict__ wsP, float2* wsZ) {
  extern __shared__ float2 st_smem[];
  const int HW = H * W, pitch = W + 1;
  float2* z = st_smem;
  float2* tw = z + H * pitch;
  double* red = (double*)(tw + max(H, W));
  const int64_t b = blockIdx.x;
  const float* __restrict__ seq = ctx + b * T * HW;
  const float* __restrict__ vy = motion + b * 2 * HW;
  const float* __restrict__ vx = vy + HW;
  float2* Z0 = wsZ + b * 2 * HW;
  float2* Z1 = Z0 + HW;
  float* Nb = wsN + b * L * 2 * HW;
  float* __restrict__ Pb = wsP + b * HW;
  const float inv = 1.f / (float)HW;

  // One loop of passes -- fill the frame, transform it, read it -- around a single inlined copy of the transform (one copy per kind of
  // pass multiplies the address arithmetic the compiler keeps live, and spills).  Kinds: 0 A_0 + i A_1 (steps 0 .. 2); 1 A_2 (AR(2));
  // 2 level l of A_0 + i A_1 (steps 4, 5); 3 level l of A_2.
  const int pre = ar == 2 ? 2 : 1, per = ar == 2 ? 2 : 1, passes = pre + per * L;
  double ms0 = 1e-30, ms1 = 1e-30, ms2 = 1e-30, g1 = 0.0;
  float mu0 = 0.f, sd0 = 0.f;
  bool dead0 = false;
  for (int pass = 0; pass < passes; ++pass) {
    const int kind = pass < pre ? pass : 2 + (pass - pre) % per, l = pass < pre ? 0 : (pass - pre) / per;
    const float* __restrict__ wl = bands + (int64_t)l * HW;
    float* N0 = Nb + (int64_t)(2 * l) * HW;
    float* N1 = N0 + HW;
    __syncthreads();                                           // the last pass has read the frame
    if (kind == 0) {
      double s[2] = {0.0, 0.0};
      ST_PIXELS(const float a0 = fmaxf(seq[(T - 1) * HW + i], thr);
                const float a1 = fmaxf(bil_fill(seq + (T - 2) * HW, H, W, (float)y - vy[i], (float)x - vx[i], 0.f), thr);
                z[li] = make_float2(a0, a1); s[0] += (double)a0 * (double)a0; s[1] += (double)a1 * (double)a1;)
      block_sum<2>(s, red);
      ms0 = fmax(s[0] / (double)HW, 1e-30), ms1 = fmax(s[1] / (double)HW, 1e-30);
    } else if (kind == 1) {
      double s[1] = {0.0};
      ST_PIXELS(const float a2 = fmaxf(bil_fill(seq + (T - 3) * HW, H, W, (float)y - 2.f * vy[i], (float)x - 2.f * vx[i], 0.f), thr);
                z[li] = make_float2(a2, 0.f); s[0] += (double)a2 * (double)a2;)
      block_sum<1>(s, red);
      ms2 = fmax(s[0] / (double)HW, 1e-30);
    } else {
      const float2* Zs = kind == 2 ? Z0 : Z1;
      ST_PIXELS(const float2 c = Zs[i]; const float w = wl[i]; z[li] = make_float2(c.x * w, -c.y * w);)
    }
    fft2d(z, tw, H, W, pitch);
    if (kind == 0) {
      // FFT(A_0)(k) = (Z(k) + conj Z(-k)) / 2; P is its modulus without the mean (the cell k = 0)
      ST_PIXELS(const int my = y ? H - y : 0, mx = x ? W - x : 0; const float2 a = z[li], c = z[my * pitch + mx];
                const float fr = 0.5f * (a.x + c.x), fi = 0.5f * (a.y - c.y);
                Z0[i] = a; Pb[i] = i ? sqrtf(fr * fr + fi * fi) : 0.f;)
      continue;
    }
    if (kind == 1) {
      ST_PIXELS(Z1[i] = z[li];)
      continue;
    }
    double mean[2], var[2], g2 = 0.0;
    frame_stats(z, H, W, pitch, inv, red, mean, var);
    if (kind == 2) {
      const bool dead1 = var[1] <= ST_DEAD * ms1;
      const float mu1 = (float)mean[1], sd1 = (float)sqrt(var[1]);
      dead0 = var[0] <= ST_DEAD * ms0, mu0 = (float)mean[0], sd0 = (float)sqrt(var[0]);
      double g[1] = {0.0};
      ST_PIXELS(const float2 c = z[li]; const float n0 = dead0 ? 0.f : (c.x * inv - mu0) / sd0, n1 = dead1 ? 0.f : (-c.y * inv - mu1) / sd1;
                N0[i] = n0; N1[i] = n1; g[0] += (double)n0 * (double)n1;)
      block_sum<1>(g, red);
      g1 = dead0 || dead1 ? 0.0 : g[0] / (double)HW;
      if (ar == 2) continue;
    } else {
      const bool dead2 = var[0] <= ST_DEAD * ms2;
      const float mu2 = (float)mean[0], sd2 = (float)sqrt(var[0]);
      double h[1] = {0.0};
      ST_PIXELS(const float n2 = dead2 ? 0.f : (z[li].x * inv - mu2) / sd2; h[0] += (double)N0[i] * (double)n2;)
      block_sum<1>(h, red);
      g2 = dead0 || dead2 ? 0.0 : h[0] / (double)HW;
    }
    if (threadIdx.x == 0) {                                    // step 5
      const double c1 = fmin(fmax(g1, -(1.0 - ST_EPS)), 1.0 - ST_EPS);
      double c2 = 0.0, p1 = c1, p2 = 0.0;
      if (ar == 2) {
        c2 = fmin(fmax(g2, 2.0 * c1 * c1 - 1.0 + ST_EPS), 1.0 - ST_EPS);
        p1 = c1 * (1.0 - c2) / (1.0 - c1 * c1), p2 = (c2 - c1 * c1) / (1.0 - c1 * c1);
      }
      const double p0 = sqrt(fmax(0.0, 1.0 - p1 * c1 - p2 * c2));
      const int64_t o = b * L + l;
      mu[o] = mu0, sigma[o] = dead0 ? 0.f : sd0;
      gamma[2 * o] = (float)c1, gamma[2 * o + 1] = (float)c2;
      phi[3 * o] = (float)p1, phi[3 * o + 1] = (float)p2, phi[3 * o + 2] = (float)p0;
    }
  }
}

// grid (M, B).  dynamic LDS as steps_analyse_kernel.  wsZn [M][B][HW] complex: conj(P FFT(z)) of the lead in hand.
// wsS [M][B][L][2][HW]: the level states; lead k writes slot k & 1.  noise may be NULL (every innovation zero: no transform runs).
__global__ void __launch_bounds__(ST_THREADS) steps_evolve_kernel(const float* __restrict__ noise, const float* __restrict__ bands,
                                                                  const float* __restrict__ mu, const float* __restrict__ sigma,
                                                                  const float* __restrict__ phi, int K, int H, int W, int L,
                                                                  const float* __restrict__ wsN, const float* __restrict__ wsP, float2* wsZn,
                                                                  float* wsS, float* __restrict__ R) {
  extern __shared__ float2 st_smem[];
  const int HW = H * W, pitch = W + 1;
  float2* z = st_smem;
  float2* tw = z + H * pitch;
  double* red = (double*)(tw + max(H, W));
  const int64_t b = blockIdx.y, mb = (int64_t)blockIdx.x * gridDim.y + b;
  const float* __restrict__ Nb = wsN + b * L * 2 * HW;
  const float* __restrict__ Pb = wsP + b * HW;
  float2* Zn = wsZn + mb * HW;
  float* S = wsS + mb * L * 2 * HW;
  const float inv = 1.f / (float)HW;

  // Per lead: pass 0 shapes the white field (step 6: conj(P FFT(z)) to the workspace), pass p >= 1 is the level pair (2 p - 2, 2 p - 1):
  // its shaped noise, the AR step and its share of the recomposition.  One inlined copy of the transform serves all passes.
  const int pairs = (L + 1) / 2;
  for (int k = 1; k <= K; ++k) {
    float* __restrict__ out = R + (mb * K + (k - 1)) * HW;    // the sum over the levels, ascending, is kept here
    for (int pass = noise ? 0 : 1; pass <= pairs; ++pass) {
      const int l0 = pass ? 2 * (pass - 1) : 0;
      const bool two = l0 + 1 < L;
      float em[2] = {0.f, 0.f}, es[2] = {0.f, 0.f};            // mean and std of e_l0, e_(l0 + 1); std 0: e_hat = 0
      if (noise) {
        __syncthreads();                                       // the last pass has read the frame
        if (pass == 0) {
          const float* __restrict__ src = noise + (mb * K + (k - 1)) * HW;
          ST_PIXELS(z[li] = make_float2(src[i], 0.f);)
        } else {
          const float* __restrict__ w0 = bands + (int64_t)l0 * HW;
          const float* __restrict__ w1 = bands + (int64_t)(two ? l0 + 1 : l0) * HW;
          // conj(w0 S + i w1 S) = conj(S) (w0 - i w1)
          ST_PIXELS(const float2 c = Zn[i]; const float a = w0[i], d = two ? w1[i] : 0.f;
                    z[li] = make_float2(c.x * a + c.y * d, c.y * a - c.x * d);)
        }
        fft2d(z, tw, H, W, pitch);
        if (pass == 0) {
          ST_PIXELS(const float2 c = z[li]; const float p = Pb[i]; Zn[i] = make_float2(c.x * p, -c.y * p);)
          continue;
        }
        double mean[2], var[2];
        frame_stats(z, H, W, pitch, inv, red, mean, var);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float sd = (float)sqrt(var[t]);
          em[t] = (float)mean[t];
          es[t] = sd > 0.f && sd < INFINITY ? sd : 0.f;        // false for a NaN
        }
      }
      // the AR step of the pair's levels and their share of R: one pass over the pixels, the running sum read and written once
      float p1[2], p2[2], p0[2], m[2], sg[2];
      const float *prev1[2], *prev2[2];                        // N^(k-1), N^(k-2): the analysis' N_l0, N_l1 until this member's states exist
      float* dst[2];                                           // lead k writes slot k & 1
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int l = two ? l0 + t : l0;
        p1[t] = phi[(b * L + l) * 3], p2[t] = phi[(b * L + l) * 3 + 1], p0[t] = phi[(b * L + l) * 3 + 2];
        m[t] = mu[b * L + l], sg[t] = sigma[b * L + l];
        prev1[t] = k == 1 ? Nb + (int64_t)(2 * l) * HW : S + (int64_t)(2 * l + ((k - 1) & 1)) * HW;
        prev2[t] = k == 1 ? Nb + (int64_t)(2 * l + 1) * HW : k == 2 ? Nb + (int64_t)(2 * l) * HW : S + (int64_t)(2 * l + (k & 1)) * HW;
        dst[t] = S + (int64_t)(2 * l + (k & 1)) * HW;
      }
      ST_PIXELS(float r = l0 ? out[i] : 0.f;
                _Pragma("unroll") for (int t = 0; t < 2; ++t) {
                  if (t == 0 || two) {
                    float eh = 0.f;
                    if (es[t] != 0.f) eh = ((t ? -z[li].y : z[li].x) * inv - em[t]) / es[t];
                    const float nw = p1[t] * prev1[t][i] + p2[t] * prev2[t][i] + p0[t] * eh;
                    dst[t][i] = nw;
                    r += m[t] + sg[t] * nw;
                  }
                }
                out[i] = r;)
    }
  }
}

// grid: M B K, lead fastest.  dynamic LDS: H W floats + ST_RED doubles.
__global__ void __launch_bounds__(ST_THREADS) steps_finish_kernel(const float* __restrict__ ctx, const float* __restrict__ motion,
                                                                  const float* __restrict__ R, float* __restrict__ out, int Bn, int T, int K,
                                                                  int H, int W, float thr, int mask, int match) {
  extern __shared__ float2 st_smem[];
  const int HW = H * W, pitch = W;
  double* red = (double*)st_smem;
  float* q = (float*)(red + ST_RED);
  const int k = (int)(blockIdx.x % K) + 1;
  const int64_t b = (blockIdx.x / K) % Bn;
  const float* __restrict__ last = ctx + (b * T + (T - 1)) * HW;
  const float* __restrict__ r = R + (int64_t)blockIdx.x * HW;
  const float* __restrict__ vy = motion + b * 2 * HW;
  const float* __restrict__ vx = vy + HW;

  double s[4] = {0.0, 0.0, 0.0, 0.0};                           // |wet0|, sum of A_0 over wet0, |S|, sum of R over S
  ST_PIXELS(const float a0 = fmaxf(last[i], thr); const bool wet = a0 > thr; const float v = mask && !wet ? thr : r[i];
            q[li] = v;
            if (wet) s[0] += 1.0, s[1] += (double)a0;
            if (v > thr) s[2] += 1.0, s[3] += (double)v;)
  block_sum<4>(s, red);
  const float shift = match && s[0] > 0.0 && s[2] > 0.0 ? (float)(s[1] / s[0] - s[3] / s[2]) : 0.f;
  ST_PIXELS(float v = q[li]; if (v > thr) v += shift; q[li] = v > thr ? v : 0.f;)
  __syncthreads();
  float* __restrict__ o = out + (int64_t)blockIdx.x * HW;
  ST_PIXELS(o[i] = bil_fill(q, H, W, (float)y - (float)k * vy[i], (float)x - (float)k * vx[i], 0.f);)
}

struct StLayout {
  int64_t n, p, z, zn, s, bytes, analyse_bytes;                  // byte offsets, each a multiple of 8 (H W is a multiple of 64)
};

bool st_layout(int64_t B, int M, int H, int W, int levels, int ar, StLayout& g) {
  if (B < 1 || B > ST_MAX_BATCH || M < 0 || M > ST_MAX_MEMBERS || (ar != 1 && ar != 2) || H < 1 || W < 1) return false;
  if (!st_frame_ok(H, W) || !st_levels_ok(H, W, levels)) return false;
  const int64_t HW = (int64_t)H * W;
  g.n = 0;
  g.p = g.n + B * levels * 2 * HW * 4;
  g.z = g.p + B * HW * 4;
  g.zn = g.analyse_bytes = g.z + B * 2 * HW * 8;
  g.s = g.zn + M * B * HW * 8;
  g.bytes = g.s + M * B * levels * 2 * HW * 4;
  return true;
}

}  // namespace

extern "C" int64_t pd_steps_ws_bytes(int64_t B, int M, int H, int W, int levels, int ar_order) {
  StLayout g;
  return st_layout(B, M, H, W, levels, ar_order, g) ? g.bytes : -1;
}

#define ST_CHECK_SHAPE(who, B, M, H, W, levels, ar, g)                                                                                      \
  PD_CHECK_ARG(st_layout(B, M, H, W, levels, ar, g),                                                                                        \
               who ": unsupported shape or options (%lld sequences, %d members, frames %d x %d, levels=%d, ar_order=%d): sides 2^a or "     \
                   "3 * 2^a, %d .. %d, H W <= %d; 2 <= levels <= floor(log2(max(H, W))) - 1; ar_order 1 or 2; B <= %d, M <= %d",             \
               (long long)(B), M, H, W, levels, ar, SP_MIN_SIDE, SP_MAX_SIDE, ST_MAX_ELEMS, ST_MAX_BATCH, ST_MAX_MEMBERS)

extern "C" int pd_steps_analyse(const float* ctx, const float* motion, const float* bands, int64_t B, int T, int H, int W, int levels,
                                int ar_order, float threshold, float* mu, float* sigma, float* phi, float* gamma, void* ws, int64_t ws_bytes,
                                pd_stream_t stream) {
  PD_CHECK_ARG(ctx && motion && bands && mu && sigma && phi && gamma && ws, "pd_steps_analyse: null pointer");
  StLayout g;
  ST_CHECK_SHAPE("pd_steps_analyse", B, 0, H, W, levels, ar_order, g);
  PD_CHECK_ARG(T >= ar_order + 1 && T <= (1 << 16), "pd_steps_analyse: %d context frames, AR(%d) needs >= %d", T, ar_order, ar_order + 1);
  PD_CHECK_ARG(threshold - threshold == 0.f, "pd_steps_analyse: threshold must be finite");
  PD_CHECK_ARG(ws_bytes >= g.analyse_bytes && ((uintptr_t)ws & 7) == 0,
               "pd_steps_analyse: the workspace holds %lld bytes (8-byte aligned), %lld are needed", (long long)ws_bytes,
               (long long)g.analyse_bytes);
  static bool lds_set[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_steps_analyse", (const void*)steps_analyse_kernel, ST_LDS_LIMIT, lds_set)) return rc;
  char* w = (char*)ws;
  hipLaunchKernelGGL(steps_analyse_kernel, dim3((unsigned)B), dim3(ST_THREADS), st_frame_lds(H, W), (hipStream_t)stream, ctx, motion, bands,
                     T, H, W, levels, ar_order, threshold, mu, sigma, phi, gamma, (float*)(w + g.n), (float*)(w + g.p), (float2*)(w + g.z));
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_steps_evolve(const float* noise, const float* bands, const float* mu, const float* sigma, const float* phi, int M, int64_t B,
                               int K, int H, int W, int levels, int ar_order, float* R, void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(bands && mu && sigma && phi && R && ws, "pd_steps_evolve: null pointer");
  PD_CHECK_ARG((const void*)R != (const void*)noise && (const void*)R != (const void*)bands && (const void*)R != (const void*)mu &&
                   (const void*)R != (const void*)sigma && (const void*)R != (const void*)phi && (const void*)R != (const void*)ws,
               "pd_steps_evolve: R aliases an input");
  StLayout g;
  ST_CHECK_SHAPE("pd_steps_evolve", B, M, H, W, levels, ar_order, g);
  PD_CHECK_ARG(M >= 1 && K >= 1 && K <= ST_MAX_LEADS, "pd_steps_evolve: %d members, %d leads (1 .. %d, 1 .. %d)", M, K, ST_MAX_MEMBERS,
               ST_MAX_LEADS);
  PD_CHECK_ARG(ws_bytes >= g.bytes && ((uintptr_t)ws & 7) == 0,
               "pd_steps_evolve: the workspace holds %lld bytes (8-byte aligned), %lld are needed", (long long)ws_bytes, (long long)g.bytes);
  static bool lds_set[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_steps_evolve", (const void*)steps_evolve_kernel, ST_LDS_LIMIT, lds_set)) return rc;
  char* w = (char*)ws;
  hipLaunchKernelGGL(steps_evolve_kernel, dim3((unsigned)M, (unsigned)B), dim3(ST_THREADS), st_frame_lds(H, W), (hipStream_t)stream, noise,
                     bands, mu, sigma, phi, K, H, W, levels, (const float*)(w + g.n), (const float*)(w + g.p), (float2*)(w + g.zn),
                     (float*)(w + g.s), R);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_steps_finish(const float* ctx, const float* motion, const float* R, float* out, int M, int64_t B, int T, int K, int H, int W,
                               float threshold, int mask, int match, pd_stream_t stream) {
  PD_CHECK_ARG(ctx && motion && R && out, "pd_steps_finish: null pointer");
  PD_CHECK_ARG(st_frame_ok(H, W), "pd_steps_finish: frames of %d x %d are not supported (sides 2^a or 3 * 2^a, %d .. %d, H W <= %d)", H, W,
               SP_MIN_SIDE, SP_MAX_SIDE, ST_MAX_ELEMS);
  PD_CHECK_ARG(M >= 1 && M <= ST_MAX_MEMBERS && B >= 1 && B <= ST_MAX_BATCH && K >= 1 && K <= ST_MAX_LEADS && T >= 1 && T <= (1 << 16),
               "pd_steps_finish: bad sizes (M=%d, B=%lld, T=%d, K=%d)", M, (long long)B, T, K);
  PD_CHECK_ARG((int64_t)M * B * K <= 0x7fffffff, "pd_steps_finish: %lld frames in one call", (long long)((int64_t)M * B * K));
  PD_CHECK_ARG(threshold - threshold == 0.f, "pd_steps_finish: threshold must be finite");
  PD_CHECK_ARG((mask == 0 || mask == 1) && (match == 0 || match == 1), "pd_steps_finish: mask %d (0 none, 1 obs), match %d (0 none, 1 mean)", mask,
               match);
  PD_CHECK_ARG((const void*)out != (const void*)R && (const void*)out != (const void*)ctx && (const void*)out != (const void*)motion,
               "pd_steps_finish: out aliases an input");
  static bool lds_set[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_steps_finish", (const void*)steps_finish_kernel, ST_LDS_LIMIT, lds_set)) return rc;
  hipLaunchKernelGGL(steps_finish_kernel, dim3((unsigned)((int64_t)M * B * K)), dim3(ST_THREADS), sizeof(float) * (size_t)H * W + sizeof(double) * ST_RED,
                     (hipStream_t)stream, ctx, motion, R, out, (int)B, T, K, H, W, threshold, mask, match);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
