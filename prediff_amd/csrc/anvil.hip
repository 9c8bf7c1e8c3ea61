// Growth / decay extrapolation (ANVIL, deterministic; DESIGN.md §7 "Growth and decay extrapolation"; prediff_amd/anvil.py, whose module
// docstring is the definition and numbers the steps; tests/_anvil_ref.py restates it).  fp32 fields, one fp64 sum (mean(A_0^2)) in the
// fixed order of block_sum, no atomics: the same input gives the same bits.
//
//   anvil_spectra_kernel  grid (2, B), 1024 threads: steps 2 and the forward half of 4.  Workgroup (q, b) builds the Lagrangian frames
//                         A_2q and A_2q+1 as ONE complex frame A_2q + i A_2q+1 in LDS (with AR(1) A_2 travels alone), transforms it and
//                         leaves the spectrum in the workspace; q = 0 also leaves max(mean(A_0^2), 1e-20).  The bands are real and even,
//                         so the inverse of w_l Z is Y_l,2q + i Y_l,2q+1.
//   anvil_cascade_kernel  grid (levels, B), 1024 threads: the rest of step 4 and steps 5 .. 8 of ONE level of one sequence -- the levels
//                         are spread over workgroups.  Two inverse transforms (the padded complex frame of steps.hip, pitch W + 1, the
//                         FFT core of fft_lds.h) give Y_l0 and D_l0 .. D_lp; a pixel i = y W + x belongs to thread i % 1024 in every
//                         pass, so Y_l1, parked in the slot of D_l1 between the two transforms, is read back by the thread that wrote
//                         it.  Then the transforms' LDS is two fp32 frames of pitch W + 1 (129 KiB at 128 x 128, exactly the complex
//                         frame): one product field D_lj D_lk at a time goes into the first, the row pass of the Gaussian window into
//                         the second, the column pass back into the first and from there to the workspace; last, gamma and phi per
//                         pixel.  A work item of a pass is a run of 8 outputs along the pass, its 8 inputs of the tap in hand in a ring
//                         of registers: one LDS read per 8 multiply-adds, the taps ascending for every output.
//                         Banks: adjacent lanes take adjacent LINES.  In the column pass the lines are columns: the lanes read 64
//                         consecutive words of a row, one per bank.  In the row pass the lines are rows and the lanes are W + 1 words
//                         apart: W + 1 is odd, so 32 lanes fall on 32 banks -- the padding column of the transform serves here too
//                         (at pitch W = 128 every lane would hit one bank).  With fewer lines than lanes (32 x 64: 32 rows) a wave
//                         spans two runs, 8 words further on: still one word per bank within each half of the wave; only frames of
//                         fewer than 32 rows see 2-way conflicts, and they are small.  The weights are staged in LDS behind the frame,
//                         padded with zeros to a multiple of 8 taps; g[d] is one address for the whole wave, a broadcast.
//   anvil_evolve_kernel   pointwise over (b, four adjacent pixels), 16-byte accesses (every side is a multiple of 4): step 9.  Reads Y_l0, D_l0,
//                         D_l1, phi1, phi2 once into registers (the level count is a template argument: every array index is a
//                         compile-time constant), loops over the leads and writes R.  No transform runs here.
// Step 10 is pd_steps_finish with one member, mask = 0, match = 0.
#include "common.h"
#include "fft_lds.h"
#include "frame_lds.h"

namespace {

constexpr int AN_MAX_RADIUS = 96;                              // ceil(3 * 32): the widest window prediff_amd/anvil.py takes
constexpr int AN_EV_THREADS = 256;
constexpr float AN_EPS = 1e-3f;
constexpr int AN_FIELDS = 5;                                   // c_00, c_11, c_01, c_22, c_02
constexpr int AN_WINDOW_LDS = (2 * AN_MAX_RADIUS + 8) / 8 * 8;    // the padded weights
constexpr int AN_RUN = 8;                                      // outputs of one work item of a window pass (the last run of a line may be shorter)

// One pass of the Gaussian window over nl lines of length N in LDS: dst(e) = sum_t gt[t] src(e - r + t), t = 0 .. 2 r ascending, an
// element outside the line adding nothing.  Element e of line l is at l * pitch + e (rows), or with COLS at e * pitch + l.  A work item is
// a run of up to AN_RUN consecutive outputs of one line, adjacent lanes taking adjacent lines; it walks the taps with the 8 elements it needs
// in a ring of registers (slot = element & 7, static because the taps are unrolled by 8): one LDS read per 8 multiply-adds.  gt: the
// weights in LDS, padded with zeros to a multiple of 8 taps, so that a block of 8 taps has no branch (a zero weight adds nothing).
template <bool COLS>
__device__ __forceinline__ void an_window_pass(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ gt, int r,
                                               int nl, int N, int pitch) {
  const int items = nl * ((N + AN_RUN - 1) / AN_RUN), taps = (2 * r + AN_RUN) / AN_RUN * AN_RUN;   // a side of 12 ends in a run of 4
  for (int w = threadIdx.x; w < items; w += ST_THREADS) {
    const int line = w % nl, e0 = (w / nl) * AN_RUN;
    const int base = COLS ? line : line * pitch, step = COLS ? pitch : 1;
    float acc[AN_RUN], ring[AN_RUN];
#pragma unroll
    for (int k = 0; k < AN_RUN; ++k) acc[k] = 0.f;
#pragma unroll
    for (int k = 0; k < AN_RUN - 1; ++k) {
      const int e = e0 - r + k;
      ring[k] = e >= 0 && e < N ? src[base + e * step] : 0.f;
    }
    for (int t0 = 0; t0 < taps; t0 += AN_RUN) {
#pragma unroll
      for (int u = 0; u < AN_RUN; ++u) {
        const int t = t0 + u, e = e0 - r + t + (AN_RUN - 1);
        ring[(u + AN_RUN - 1) % AN_RUN] = e >= 0 && e < N ? src[base + e * step] : 0.f;
        const float gw = gt[t];
#pragma unroll
        for (int o = 0; o < AN_RUN; ++o) acc[o] += gw * ring[(u + o) % AN_RUN];
      }
    }
#pragma unroll
    for (int o = 0; o < AN_RUN; ++o)
      if (e0 + o < N) dst[base + (e0 + o) * step] = acc[o];
  }
}

// grid (2, B).  dynamic LDS: (H (W + 1) + max(H, W)) complex + ST_RED doubles.  wsZ [B][2][HW] complex, wsMs [B].
__global__ void __launch_bounds__(ST_THREADS) anvil_spectra_kernel(const float* __restrict__ ctx, const float* __restrict__ motion, int T,
                                                                   int H, int W, int ar, float2* __restrict__ wsZ,
                                                                   double* __restrict__ wsMs) {
  extern __shared__ float2 st_smem[];
  const int HW = H * W, pitch = W + 1;
  float2* z = st_smem;
  float2* tw = z + H * pitch;
  double* red = (double*)(tw + max(H, W));
  const int q = blockIdx.x;
  const int64_t b = blockIdx.y;
  const float* __restrict__ seq = ctx + b * T * HW;
  const float* __restrict__ vy = motion + b * 2 * HW;
  const float* __restrict__ vx = vy + HW;
  float2* __restrict__ Zq = wsZ + (b * 2 + q) * HW;
  const int j0 = 2 * q, j1 = 2 * q + 1;
  const bool two = j1 <= ar + 1;
  const float* __restrict__ f0 = seq + (int64_t)(T - 1 - j0) * HW;
  const float* __restrict__ f1 = seq + (int64_t)(T - 1 - (two ? j1 : j0)) * HW;
  const float l0 = (float)j0, l1 = (float)j1;

  double s[1] = {0.0};
  ST_PIXELS(const float a0 = q == 0 ? f0[i] : bil_fill(f0, H, W, (float)y - l0 * vy[i], (float)x - l0 * vx[i], 0.f);
            const float a1 = two ? bil_fill(f1, H, W, (float)y - l1 * vy[i], (float)x - l1 * vx[i], 0.f) : 0.f;
            z[li] = make_float2(a0, a1); s[0] += (double)a0 * (double)a0;)
  if (q == 0) {
    block_sum<1>(s, red);
    if (threadIdx.x == 0) wsMs[b] = fmax(s[0] / (double)HW, 1e-20);
  }
  fft2d(z, tw, H, W, pitch);
  ST_PIXELS(Zq[i] = z[li];)
}

// grid (L, B).  dynamic LDS as anvil_spectra_kernel + AN_WINDOW_LDS floats.  wsY [B][L][HW]: Y_l0.  wsD [B][L][3][HW]: D_l0, D_l1, D_l2 (AR(2) only).
// wsC [B][L][5][HW]: the windowed moments.  window: g[-r .. r].  phi, gamma [B][L][2][HW].
__global__ void __launch_bounds__(ST_THREADS) anvil_cascade_kernel(const float* __restrict__ bands, const float* __restrict__ window, int r,
                                                                   double w0, int H, int W, int L, int ar,
                                                                   const float2* __restrict__ wsZ, const double* __restrict__ wsMs,
                                                                   float* __restrict__ wsY, float* wsD, float* wsC,
                                                                   float* __restrict__ phi, float* __restrict__ gamma) {
  extern __shared__ float2 st_smem[];
  const int HW = H * W, pitch = W + 1;
  float2* z = st_smem;
  float2* tw = z + H * pitch;
  const int l = blockIdx.x;
  const int64_t b = blockIdx.y, bl = b * L + l;
  const float2* __restrict__ Zb = wsZ + b * 2 * HW;
  const float* __restrict__ wl = bands + (int64_t)l * HW;
  float* __restrict__ Y0 = wsY + bl * HW;
  float* D = wsD + bl * 3 * HW;
  float* C = wsC + bl * AN_FIELDS * HW;
  const float inv = 1.f / (float)HW;

  // steps 4, 5: the inverse of w_l Z_q is the forward transform of its conjugate, conjugated and scaled
  for (int q = 0; q < 2; ++q) {
    __syncthreads();                                           // the last pass has read the frame
    ST_PIXELS(const float2 c = Zb[q * HW + i]; const float w = wl[i]; z[li] = make_float2(c.x * w, -c.y * w);)
    fft2d(z, tw, H, W, pitch);
    if (q == 0) {
      ST_PIXELS(const float2 c = z[li]; const float y0 = c.x * inv, y1 = -c.y * inv; Y0[i] = y0; D[i] = y0 - y1; D[HW + i] = y1;)
    } else {
      ST_PIXELS(const float2 c = z[li]; const float y2 = c.x * inv, y3 = -c.y * inv; D[HW + i] = D[HW + i] - y2;
                if (ar == 2) D[2 * HW + i] = y2 - y3;)
    }
  }

  // step 6: one product field at a time, rows then columns, taps ascending; a tap outside the frame is left out
  float* fa = (float*)st_smem;
  float* fb = fa + H * pitch;
  float* gl = (float*)((double*)(tw + max(H, W)) + ST_RED);
  const int nf = ar == 2 ? AN_FIELDS : 3;
  for (int t = threadIdx.x; t < (2 * r + AN_RUN) / AN_RUN * AN_RUN; t += ST_THREADS) gl[t] = t <= 2 * r ? window[t] : 0.f;
  __syncthreads();                                             // the transforms have read the LDS
  for (int f = 0; f < nf; ++f) {
    const int ja = f == 1 ? 1 : f == 3 ? 2 : 0, jb = f == 0 ? 0 : f == 3 || f == 4 ? 2 : 1;      // (0,0) (1,1) (0,1) (2,2) (0,2)
    ST_PIXELS(fa[li] = D[ja * HW + i] * D[jb * HW + i];)
    __syncthreads();
    an_window_pass<false>(fa, fb, gl, r, H, W, pitch);
    __syncthreads();
    an_window_pass<true>(fb, fa, gl, r, W, H, pitch);
    __syncthreads();
    ST_PIXELS(C[f * HW + i] = fa[li];)                         // the pixel this thread fills again for the next field
  }

  // steps 7, 8
  const float delta = (float)(1e-6 * w0 * wsMs[b]);
  float* __restrict__ ph = phi + bl * 2 * HW;
  float* __restrict__ ga = gamma + bl * 2 * HW;
  ST_PIXELS(const float s0 = sqrtf(C[i] + delta);
            float g1 = C[2 * HW + i] / (s0 * sqrtf(C[HW + i] + delta));
            g1 = fminf(fmaxf(g1, -(1.f - AN_EPS)), 1.f - AN_EPS);
            float g2 = 0.f, p1 = g1, p2 = 0.f;
            if (ar == 2) {
              g2 = C[4 * HW + i] / (s0 * sqrtf(C[3 * HW + i] + delta));
              g2 = fminf(fmaxf(g2, 2.f * g1 * g1 - 1.f + AN_EPS), 1.f - AN_EPS);
              const float den = 1.f - g1 * g1;
              p1 = g1 * (1.f - g2) / den;
              p2 = (g2 - g1 * g1) / den;
            }
            ga[i] = g1; ga[HW + i] = g2; ph[i] = p1; ph[HW + i] = p2;)
}

__device__ __forceinline__ float4 an_fma(float4 a, float4 b, float4 c) {
  return make_float4(a.x * b.x + c.x, a.y * b.y + c.y, a.z * b.z + c.z, a.w * b.w + c.w);
}
__device__ __forceinline__ float4 an_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// grid (ceil(HW / 4 / 256), B).  Everything in units of four pixels.
template <int L>
__global__ void __launch_bounds__(AN_EV_THREADS) anvil_evolve_kernel(const float4* __restrict__ phi, const float4* __restrict__ wsY,
                                                                     const float4* __restrict__ wsD, float4* __restrict__ R, int K,
                                                                     int HW4) {
  const int p = blockIdx.x * AN_EV_THREADS + threadIdx.x;
  if (p >= HW4) return;
  const int64_t b = blockIdx.y;
  float4 Y[L], d1[L], d2[L], p1[L], p2[L];
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int64_t bl = b * L + l;
    Y[l] = wsY[bl * HW4 + p];
    d1[l] = wsD[(bl * 3) * HW4 + p], d2[l] = wsD[(bl * 3 + 1) * HW4 + p];
    p1[l] = phi[(bl * 2) * HW4 + p], p2[l] = phi[(bl * 2 + 1) * HW4 + p];
  }
  for (int k = 0; k < K; ++k) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const float4 t = make_float4(p2[l].x * d2[l].x, p2[l].y * d2[l].y, p2[l].z * d2[l].z, p2[l].w * d2[l].w);
      const float4 d = an_fma(p1[l], d1[l], t);
      d2[l] = d1[l], d1[l] = d;
      Y[l] = an_add(Y[l], d);
      r = an_add(r, Y[l]);
    }
    R[(b * K + k) * HW4 + p] = r;
  }
}

struct AnLayout {
  int64_t z, ms, y, d, c, bytes;                                 // byte offsets, each a multiple of 16 (H W is a multiple of 16)
};

bool an_layout(int64_t B, int H, int W, int levels, int ar, AnLayout& g) {
  if (B < 1 || B > ST_MAX_BATCH || (ar != 1 && ar != 2) || H < 1 || W < 1) return false;
  if (!st_frame_ok(H, W) || !st_levels_ok(H, W, levels)) return false;
  const int64_t HW = (int64_t)H * W;
  g.z = 0;
  g.ms = g.z + B * 2 * HW * 8;
  g.y = g.ms + (B * 8 + 15) / 16 * 16;
  g.d = g.y + B * levels * HW * 4;
  g.c = g.d + B * levels * 3 * HW * 4;
  g.bytes = g.c + B * levels * AN_FIELDS * HW * 4;
  return true;
}

template <int L>
void an_launch_evolve(const float* phi, const char* w, const AnLayout& g, float* R, int64_t B, int K, int HW, hipStream_t stream) {
  const int HW4 = HW / 4;
  hipLaunchKernelGGL(anvil_evolve_kernel<L>, dim3((unsigned)((HW4 + AN_EV_THREADS - 1) / AN_EV_THREADS), (unsigned)B), dim3(AN_EV_THREADS), 0,
                     stream, (const float4*)phi, (const float4*)(w + g.y), (const float4*)(w + g.d), (float4*)R, K, HW4);
}

}  // namespace

extern "C" int64_t pd_anvil_ws_bytes(int64_t B, int H, int W, int levels, int ar_order) {
  AnLayout g;
  return an_layout(B, H, W, levels, ar_order, g) ? g.bytes : -1;
}

#define AN_CHECK_SHAPE(who, B, H, W, levels, ar, g)                                                                                          \
  PD_CHECK_ARG(an_layout(B, H, W, levels, ar, g),                                                                                           \
               who ": unsupported shape or options (%lld sequences, frames %d x %d, levels=%d, ar_order=%d): sides 2^a or 3 * 2^a, "        \
                   "%d .. %d, H W <= %d; 2 <= levels <= floor(log2(max(H, W))) - 1; ar_order 1 or 2; B <= %d",                               \
               (long long)(B), H, W, levels, ar, SP_MIN_SIDE, SP_MAX_SIDE, ST_MAX_ELEMS, ST_MAX_BATCH)

extern "C" int pd_anvil_analyse(const float* ctx, const float* motion, const float* bands, const float* window, int radius,
                                double window_sum_sq, int64_t B, int T, int H, int W, int levels, int ar_order, float* phi, float* gamma,
                                void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(ctx && motion && bands && window && phi && gamma && ws, "pd_anvil_analyse: null pointer");
  AnLayout g;
  AN_CHECK_SHAPE("pd_anvil_analyse", B, H, W, levels, ar_order, g);
  PD_CHECK_ARG(T >= ar_order + 2 && T <= (1 << 16), "pd_anvil_analyse: %d context frames, AR(%d) on first differences needs >= %d", T,
               ar_order, ar_order + 2);
  PD_CHECK_ARG(radius >= 1 && radius <= AN_MAX_RADIUS, "pd_anvil_analyse: window radius %d (1 .. %d)", radius, AN_MAX_RADIUS);
  PD_CHECK_ARG(window_sum_sq > 0.0 && window_sum_sq - window_sum_sq == 0.0, "pd_anvil_analyse: window_sum_sq must be positive and finite");
  PD_CHECK_ARG(ws_bytes >= g.bytes && ((uintptr_t)ws & 15) == 0,
               "pd_anvil_analyse: the workspace holds %lld bytes (16-byte aligned), %lld are needed", (long long)ws_bytes,
               (long long)g.bytes);
  PD_CHECK_ARG((const void*)phi != (const void*)gamma && (const void*)phi != (const void*)ws && (const void*)gamma != (const void*)ws &&
                   (const void*)phi != (const void*)ctx && (const void*)gamma != (const void*)ctx && (const void*)phi != (const void*)motion &&
                   (const void*)gamma != (const void*)motion,
               "pd_anvil_analyse: an output aliases an input");
  static bool lds_spectra[PD_MAX_DEVICES], lds_cascade[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_anvil_analyse", (const void*)anvil_spectra_kernel, ST_LDS_LIMIT, lds_spectra)) return rc;
  if (int rc = pd_raise_lds("pd_anvil_analyse", (const void*)anvil_cascade_kernel, ST_LDS_LIMIT, lds_cascade)) return rc;
  char* w = (char*)ws;
  hipLaunchKernelGGL(anvil_spectra_kernel, dim3(2, (unsigned)B), dim3(ST_THREADS), st_frame_lds(H, W), (hipStream_t)stream, ctx, motion, T, H,
                     W, ar_order, (float2*)(w + g.z), (double*)(w + g.ms));
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(anvil_cascade_kernel, dim3((unsigned)levels, (unsigned)B), dim3(ST_THREADS),
                     st_frame_lds(H, W) + sizeof(float) * AN_WINDOW_LDS, (hipStream_t)stream,
                     bands, window, radius, window_sum_sq, H, W, levels, ar_order, (const float2*)(w + g.z), (const double*)(w + g.ms),
                     (float*)(w + g.y), (float*)(w + g.d), (float*)(w + g.c), phi, gamma);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_anvil_evolve(const float* phi, int64_t B, int K, int H, int W, int levels, int ar_order, float* R, const void* ws,
                               int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(phi && R && ws, "pd_anvil_evolve: null pointer");
  PD_CHECK_ARG((const void*)R != (const void*)phi && (const void*)R != ws, "pd_anvil_evolve: R aliases an input");
  AnLayout g;
  AN_CHECK_SHAPE("pd_anvil_evolve", B, H, W, levels, ar_order, g);
  PD_CHECK_ARG(K >= 1 && K <= ST_MAX_LEADS, "pd_anvil_evolve: %d leads (1 .. %d)", K, ST_MAX_LEADS);
  PD_CHECK_ARG(ws_bytes >= g.bytes && ((uintptr_t)ws & 15) == 0,
               "pd_anvil_evolve: the workspace holds %lld bytes (16-byte aligned), %lld are needed", (long long)ws_bytes, (long long)g.bytes);
  PD_CHECK_ARG(((uintptr_t)phi & 15) == 0 && ((uintptr_t)R & 15) == 0, "pd_anvil_evolve: phi and R must be 16-byte aligned");
  const char* w = (const char*)ws;
  const int HW = H * W;
  hipStream_t s = (hipStream_t)stream;
  switch (levels) {
    case 2: an_launch_evolve<2>(phi, w, g, R, B, K, HW, s); break;
    case 3: an_launch_evolve<3>(phi, w, g, R, B, K, HW, s); break;
    case 4: an_launch_evolve<4>(phi, w, g, R, B, K, HW, s); break;
    case 5: an_launch_evolve<5>(phi, w, g, R, B, K, HW, s); break;
    case 6: an_launch_evolve<6>(phi, w, g, R, B, K, HW, s); break;
    case 7: an_launch_evolve<7>(phi, w, g, R, B, K, HW, s); break;
    default: an_launch_evolve<8>(phi, w, g, R, B, K, HW, s); break;
  }
  PD_CHECK_LAUNCH();
  return PD_OK;
}
