// Pooled SEVIR skill counts and ensemble verification scores (CRPS, fair CRPS, Brier, ensemble-mean RMSE, spread), read in place.
//
// Both entry points take the sizes of the N, T, H, W, C axes and the element strides of every operand, so any 5-letter layout (and,
// with size-1 / stride-0 axes, the 4-letter ones) is read where it lies: no permuted copy and no pooled copy is made.  Pooling is the
// reference's F.max_pool2d over (H, W) with kernel = stride = s for each (N, T, C) (floor mode: rows / columns that do not fill a window
// are dropped, a NaN anywhere in a window makes the cell NaN), applied to the raw values; the cell is then divided by `divisor` with an
// IEEE division.  Division by a positive constant is monotone, so max-then-divide equals the reference's divide-then-max bit for bit.
//
// pd_sevir_skill_counts_pooled: hits / misses / false alarms of the pooled cells, the same int64 counters as pd_sevir_skill_counts.
// pd_ensemble_score_update (not in the reference): per pooled pixel with target y and members x_1..x_M (valid when none is NaN)
//   sum_i |x_i - y|, sum_ij |x_i - x_j|, (mean - y)^2, sum_i (x_i - mean)^2 / (M - 1)   -> fp64 sums [4][T]
//   (c - M o)^2 with c = #{x_i >= thr}, o = [y >= thr]                                -> exact int64 [thr][T]
//   1                                                                                  -> int64 n_valid [T]
// A block takes P pixels of one (n, t) slab, stages their M member values in LDS (each read from memory once) and gives every pixel
// G = 256 / P threads; the pairwise term is M (M - 1) / 2 LDS differences per pixel.  The floating sums are reduced deterministically:
// fixed-order per-pixel and per-block trees, per-block partials in a workspace, and a fixed-order final pass per (t, sum) -- no float
// atomics, so the same inputs give the same bits.  Integer counters use int64 atomics (order independent).
#include "axes.h"
#include "common.h"

namespace {

constexpr int ES_MAXTHR = 8;
constexpr int ES_MAXM = 512;           // members (8 GPUs x 64)
constexpr int ES_TILE_FLOATS = 8192;   // LDS member tile: P * M floats (32 KB)
constexpr int ES_THREADS = 256;

struct Geom : Axes5 {        // pooled sizes: h = H / s, w = W / s
  int s;
};

// the pooled value of cell (ho, wo) of the (n, t, c) plane at `base`: max over the s x s window, NaN if any element is NaN
__device__ __forceinline__ float pooled(const float* __restrict__ base, const Axes5& st, int64_t ho, int64_t wo, int s, float divisor) {
  float m = -INFINITY;
  bool nan = false;
  for (int dh = 0; dh < s; ++dh) {
    const float* row = base + (ho * s + dh) * st.h + wo * s * st.w;
    for (int dw = 0; dw < s; ++dw) {
      const float v = row[dw * st.w];
      nan |= isnan(v);
      m = fmaxf(m, v);
    }
  }
  return nan ? NAN : m / divisor;      // IEEE division, as data.float() / scale in the reference
}

// ----------------------------------------------------------------------------------------------------------- pooled skill counts
// grid (chunks, slabs): a block stays inside one (n, t) slab of ho * wo * c cells and walks the slabs with a grid stride.
__global__ void __launch_bounds__(256) sevir_skill_pooled_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                 const float* __restrict__ thr, int nthr, float divisor,
                                                                 long long* __restrict__ counts, Geom g, Axes5 sp, Axes5 stt,
                                                                 int keep_seq) {
  float th[ES_MAXTHR];
#pragma unroll
  for (int k = 0; k < ES_MAXTHR; ++k) th[k] = k < nthr ? thr[k] : 3.0e38f;
  const int lane = threadIdx.x & 63;
  const int64_t nslab = g.n * g.t, ncell = g.h * g.w * g.c;
  for (int64_t slab = blockIdx.y; slab < nslab; slab += gridDim.y) {
    const int64_t n = slab / g.t, t = slab % g.t;
    int h[ES_MAXTHR], ms[ES_MAXTHR], fa[ES_MAXTHR];
#pragma unroll
    for (int k = 0; k < ES_MAXTHR; ++k) h[k] = ms[k] = fa[k] = 0;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < ncell; q += (int64_t)gridDim.x * 256) {
      const int64_t c = q % g.c, wo = (q / g.c) % g.w, ho = q / (g.c * g.w);
      const float pv = pooled(pred + n * sp.n + t * sp.t + c * sp.c, sp, ho, wo, g.s, divisor);
      const float tv = pooled(target + n * stt.n + t * stt.t + c * stt.c, stt, ho, wo, g.s, divisor);
      const bool ok = !(isnan(pv) || isnan(tv));
#pragma unroll
      for (int k = 0; k < ES_MAXTHR; ++k) {
        const bool tb = ok && tv >= th[k], pb = ok && pv >= th[k];
        h[k] += tb && pb;
        ms[k] += tb && !pb;
        fa[k] += !tb && pb;
      }
    }
    const int64_t tk = keep_seq ? t : 0, Tk = keep_seq ? g.t : 1;
#pragma unroll
    for (int k = 0; k < ES_MAXTHR; ++k) {
      if (k >= nthr) break;
      int a = h[k], b = ms[k], c = fa[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64); }
      if (lane == 0) {
        long long* dst = counts + ((int64_t)k * Tk + tk) * 3;
        if (a) atomicAdd((unsigned long long*)dst, (unsigned long long)a);
        if (b) atomicAdd((unsigned long long*)(dst + 1), (unsigned long long)b);
        if (c) atomicAdd((unsigned long long*)(dst + 2), (unsigned long long)c);
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------------- ensemble scores
// One block per tile of P pixels (P a power of two, P * M <= ES_TILE_FLOATS): block b covers cells [tile * P, tile * P + P) of slab
// b / tiles, slab = n * T + t.  Thread tid serves pixel p = tid % P as member-row group j = tid / P (G = 256 / P groups per pixel).
// ws[b * 4 + k]: the block's fp64 partial of sum k.
__global__ void __launch_bounds__(ES_THREADS) ensemble_score_kernel(const float* __restrict__ ens, const float* __restrict__ target,
                                                                    const float* __restrict__ thr, int nthr, float divisor, int M,
                                                                    int64_t ens_stride_m, Geom g, Axes5 se, Axes5 stt, int P,
                                                                    int64_t tiles, int keep_seq, long long* __restrict__ n_valid,
                                                                    long long* __restrict__ brier, double* __restrict__ ws) {
  extern __shared__ float xs[];                      // [M][P] member values of the tile
  __shared__ float ys[ES_THREADS];
  __shared__ int bad[ES_THREADS];
  __shared__ double mean_s[ES_THREADS];
  __shared__ double red[4][ES_THREADS];
  __shared__ int cred[ES_MAXTHR][ES_THREADS];
  __shared__ unsigned long long bsum[ES_MAXTHR + 1];  // brier sums of the block, [ES_MAXTHR]: valid pixels

  const int tid = threadIdx.x;
  const int G = ES_THREADS / P;
  const int p = tid % P, j = tid / P;
  const int64_t b = blockIdx.x;
  const int64_t slab = b / tiles, tile = b % tiles;
  const int64_t n = slab / g.t, t = slab % g.t;
  const int64_t ncell = g.h * g.w * g.c, cell0 = tile * P;

  float th[ES_MAXTHR];
#pragma unroll
  for (int k = 0; k < ES_MAXTHR; ++k) th[k] = k < nthr ? thr[k] : 3.0e38f;

  if (tid <= ES_MAXTHR) bsum[tid] = 0;
  if (tid < P) bad[tid] = cell0 + tid >= ncell ? 1 : 0;   // cells past the end of the slab
  __syncthreads();
  // member values (m < M) and the target (m == M): the s x s window of a cell is read by a group of L lanes (L: the largest power of
  // two <= min(s, 16); lane l takes columns l, l + L, ... of every window row) and folded with shuffles (few lanes per window: the
  // shuffles cost more than the loads they spread); the trip count is uniform so the lane groups stay whole
  int L = 1;
  while (L * 2 <= min(g.s, 16)) L *= 2;
  const int total = (M + 1) * P * L;
  for (int base = 0; base < total; base += ES_THREADS) {
    const int i = base + tid;
    const int cell = i / L, l = i % L;
    const int pp = cell % P, m = cell / P;
    const int64_t q = cell0 + pp;
    const bool act = i < total && q < ncell;
    float mx = -INFINITY;
    int nan = 0;
    if (act) {
      const int64_t c = q % g.c, wo = (q / g.c) % g.w, ho = q / (g.c * g.w);
      const Axes5& st = m < M ? se : stt;
      const float* src = m < M ? ens + m * ens_stride_m + n * se.n + t * se.t + c * se.c : target + n * stt.n + t * stt.t + c * stt.c;
      for (int dh = 0; dh < g.s; ++dh) {
        const float* row = src + (ho * g.s + dh) * st.h + wo * g.s * st.w;
        for (int dw = l; dw < g.s; dw += L) {
          const float v = row[dw * st.w];
          nan |= isnan(v) ? 1 : 0;
          mx = fmaxf(mx, v);
        }
      }
    }
    for (int o = 1; o < L; o <<= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      nan |= __shfl_xor(nan, o, 64);
    }
    if (i < total && l == 0) {
      const float v = act && !nan ? mx / divisor : 0.0f;   // IEEE division, as data.float() / scale in the reference
      if (m < M) xs[cell] = v;
      else ys[pp] = v;
      if (act && nan) atomicOr(&bad[pp], 1);
    }
  }
  __syncthreads();

  // phase 1: per thread over its blocks of four member rows (rows 4 rb .. 4 rb + 3 for rb = j, j + G, ...): sum x, sum |x - y|, threshold
  // counts, and the pairwise sum over k > i -- each x_k read from LDS serves the four rows of the block
  const bool ok = !bad[p];
  double sx = 0.0, sab = 0.0, pr = 0.0;
  int cnt[ES_MAXTHR];
#pragma unroll
  for (int k = 0; k < ES_MAXTHR; ++k) cnt[k] = 0;
  const float y = ys[p];
  if (ok) {
    for (int r0 = 4 * j; r0 < M; r0 += 4 * G) {
      const int nr = min(4, M - r0);
      for (int a = 0; a < nr; ++a) {
        const float xi = xs[(r0 + a) * P + p];
        sx += (double)xi;
        sab += fabs((double)xi - (double)y);
#pragma unroll
        for (int k = 0; k < ES_MAXTHR; ++k) cnt[k] += xi >= th[k];
      }
      if (nr == 4) {
        const float x0 = xs[r0 * P + p], x1 = xs[(r0 + 1) * P + p], x2 = xs[(r0 + 2) * P + p], x3 = xs[(r0 + 3) * P + p];
        pr += (double)(fabsf(x0 - x1) + fabsf(x0 - x2) + fabsf(x0 - x3) + fabsf(x1 - x2) + fabsf(x1 - x3) + fabsf(x2 - x3));
        for (int k0 = r0 + 4; k0 < M; k0 += 32) {    // fp32 over at most 128 differences, fp64 across chunks
          const int k1 = min(M, k0 + 32);
          float acc = 0.0f;
          for (int k = k0; k < k1; ++k) {
            const float xk = xs[k * P + p];
            acc += (fabsf(x0 - xk) + fabsf(x1 - xk)) + (fabsf(x2 - xk) + fabsf(x3 - xk));
          }
          pr += (double)acc;
        }
      } else {                                        // the last M % 4 rows: only the pairs among themselves remain
        for (int a = 0; a < nr; ++a)
          for (int b2 = a + 1; b2 < nr; ++b2) pr += (double)fabsf(xs[(r0 + a) * P + p] - xs[(r0 + b2) * P + p]);
      }
    }
  }
  red[0][tid] = sx;
  red[1][tid] = sab;
  red[2][tid] = pr;
#pragma unroll
  for (int k = 0; k < ES_MAXTHR; ++k) cred[k][tid] = cnt[k];
  __syncthreads();
  double sx_t = 0.0, sab_t = 0.0, pr_t = 0.0;
  int cnt_t[ES_MAXTHR];
#pragma unroll
  for (int k = 0; k < ES_MAXTHR; ++k) cnt_t[k] = 0;
  if (tid < P) {                                    // fixed order over the pixel's G row groups
    for (int jj = 0; jj < G; ++jj) {
      sx_t += red[0][jj * P + p];
      sab_t += red[1][jj * P + p];
      pr_t += red[2][jj * P + p];
#pragma unroll
      for (int k = 0; k < ES_MAXTHR; ++k) cnt_t[k] += cred[k][jj * P + p];
    }
    mean_s[p] = sx_t / (double)M;
  }
  __syncthreads();

  // phase 2: sum of squared deviations from the ensemble mean
  const double mean = mean_s[p];
  double sv = 0.0;
  if (ok)
    for (int i = j; i < M; i += G) {
      const double d = (double)xs[i * P + p] - mean;
      sv += d * d;
    }
  red[3][tid] = sv;
  __syncthreads();
  double e[4] = {0.0, 0.0, 0.0, 0.0};
  if (tid < P) {
    double sv_t = 0.0;
    for (int jj = 0; jj < G; ++jj) sv_t += red[3][jj * P + p];
    if (ok) {
      const double dm = mean - (double)y;
      e[0] = sab_t;
      e[1] = 2.0 * pr_t;
      e[2] = dm * dm;
      e[3] = M > 1 ? sv_t / (double)(M - 1) : 0.0;
#pragma unroll
      for (int k = 0; k < ES_MAXTHR; ++k) {
        if (k >= nthr) break;
        const long long d = (long long)cnt_t[k] - (y >= th[k] ? (long long)M : 0ll);
        if (d) atomicAdd(&bsum[k], (unsigned long long)(d * d));
      }
      atomicAdd(&bsum[ES_MAXTHR], 1ull);
    }
  }
  __syncthreads();                                   // everyone is done reading red[]
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][tid] = e[k];  // zero for tid >= P and invalid pixels
  __syncthreads();
  for (int h = ES_THREADS / 2; h > 0; h >>= 1) {    // fixed-order tree over the block
    if (tid < h) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + h];
    }
    __syncthreads();
  }
  if (tid < 4) ws[b * 4 + tid] = red[tid][0];
  const int64_t Tk = keep_seq ? g.t : 1, tk = keep_seq ? t : 0;
  if (tid < nthr && bsum[tid]) atomicAdd((unsigned long long*)(brier + (int64_t)tid * Tk + tk), bsum[tid]);
  if (tid == ES_MAXTHR && bsum[ES_MAXTHR]) atomicAdd((unsigned long long*)(n_valid + tk), bsum[ES_MAXTHR]);
}

// grid (T_out, 4): sum k of step t over the blocks of that step, in a fixed order, added to sums[k][t]
__global__ void __launch_bounds__(256) ensemble_score_final_kernel(const double* __restrict__ ws, int64_t N, int64_t T, int64_t tiles,
                                                                   int keep_seq, double* __restrict__ sums) {
  __shared__ double r[256];
  const int tk = blockIdx.x, k = blockIdx.y;
  const int Tk = keep_seq ? (int)T : 1;
  // the blocks of step tk: (n, t = tk, tile) for keep_seq, every block otherwise
  const int64_t per_t = keep_seq ? N * tiles : N * T * tiles;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < per_t; i += 256) {
    int64_t b;
    if (keep_seq) {
      const int64_t n = i / tiles, tile = i % tiles;
      b = (n * T + tk) * tiles + tile;
    } else {
      b = i;
    }
    a += ws[b * 4 + k];
  }
  r[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) r[threadIdx.x] += r[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[(int64_t)k * Tk + tk] += r[0];
}

bool read_geom(const int64_t* sizes, int s, Geom& g) {
  if (s < 1 || !read_axes(sizes, g)) return false;
  g.h /= s;
  g.w /= s;
  g.s = s;
  return true;
}

// pixels per block: the largest power of two with P * M <= ES_TILE_FLOATS, halved (down to 1) while the update gives fewer than 1024
// blocks (pooled frames, one context) -- more threads per pixel and more blocks reading the windows instead of idle CUs
int tile_pixels(int M, int64_t nslab, int64_t ncell) {
  int P = ES_THREADS;
  while (P > 1 && P * M > ES_TILE_FLOATS) P >>= 1;
  while (P > 1 && nslab * ((ncell + P - 1) / P) < 1024) P >>= 1;
  return P;
}

}  // namespace

extern "C" int pd_sevir_skill_counts_pooled(const float* pred, const float* target, const float* thresholds, int nthr, float divisor,
                                            long long* counts, const int64_t* sizes, const int64_t* pred_strides,
                                            const int64_t* target_strides, int pool, int keep_seq, pd_stream_t stream) {
  PD_CHECK_ARG(pred && target && thresholds && counts && pred_strides && target_strides, "pd_sevir_skill_counts_pooled: null pointer");
  Geom g;
  PD_CHECK_ARG(read_geom(sizes, pool, g) && nthr > 0 && nthr <= ES_MAXTHR, "pd_sevir_skill_counts_pooled: bad sizes / pool / thresholds");
  const int64_t ncell = g.h * g.w * g.c, nslab = g.n * g.t;
  PD_CHECK_ARG(ncell * nslab < (1ll << 40), "pd_sevir_skill_counts_pooled: more than 2^40 cells in one update");
  if (ncell == 0) return PD_OK;                     // a pool larger than the frame: no cell, nothing counted
  const unsigned chunks = (unsigned)std::min((int64_t)64, (ncell + 255) / 256);
  const unsigned gy = (unsigned)std::min(nslab, (int64_t)16384);
  hipLaunchKernelGGL(sevir_skill_pooled_kernel, dim3(chunks, gy), dim3(256), 0, (hipStream_t)stream, pred, target, thresholds, nthr,
                     divisor, counts, g, read_strides(pred_strides), read_strides(target_strides), keep_seq);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int64_t pd_ensemble_score_ws_doubles(int M, const int64_t* sizes, int pool) {
  Geom g;
  if (M < 1 || M > ES_MAXM || !read_geom(sizes, pool, g)) return -1;
  const int64_t ncell = g.h * g.w * g.c, P = tile_pixels(M, g.n * g.t, ncell);
  return std::max<int64_t>(1, g.n * g.t * ((ncell + P - 1) / P) * 4);
}

extern "C" int pd_ensemble_score_update(const float* ens, const float* target, const float* thresholds, int nthr, float divisor, int M,
                                        const int64_t* sizes, const int64_t* ens_strides, const int64_t* target_strides, int pool,
                                        int keep_seq, long long* n_valid, long long* brier, double* sums, double* ws, int64_t ws_doubles,
                                        pd_stream_t stream) {
  PD_CHECK_ARG(ens && target && thresholds && n_valid && brier && sums && ws && ens_strides && target_strides,
               "pd_ensemble_score_update: null pointer");
  PD_CHECK_ARG(M >= 1 && M <= ES_MAXM, "pd_ensemble_score_update: %d members (supported: 1 .. %d)", M, ES_MAXM);
  Geom g;
  PD_CHECK_ARG(read_geom(sizes, pool, g) && nthr > 0 && nthr <= ES_MAXTHR, "pd_ensemble_score_update: bad sizes / pool / thresholds");
  const int64_t ncell = g.h * g.w * g.c;
  const int P = tile_pixels(M, g.n * g.t, ncell);
  const int64_t tiles = (ncell + P - 1) / P, nblocks = g.n * g.t * tiles;
  PD_CHECK_ARG(ws_doubles >= nblocks * 4, "pd_ensemble_score_update: workspace of %lld doubles < %lld", (long long)ws_doubles,
               (long long)(nblocks * 4));
  PD_CHECK_ARG(nblocks < (1ll << 24), "pd_ensemble_score_update: too many pixels in one update");
  if (nblocks == 0) return PD_OK;                   // a pool larger than the frame: no pixel
  hipLaunchKernelGGL(ensemble_score_kernel, dim3((unsigned)nblocks), dim3(ES_THREADS), (size_t)P * M * sizeof(float), (hipStream_t)stream,
                     ens, target, thresholds, nthr, divisor, M, ens_strides[0], g, read_strides(ens_strides + 1),
                     read_strides(target_strides), P, tiles, keep_seq, n_valid, brier, ws);
  PD_CHECK_LAUNCH();
  const int Tk = keep_seq ? (int)g.t : 1;
  hipLaunchKernelGGL(ensemble_score_final_kernel, dim3((unsigned)Tk, 4), dim3(256), 0, (hipStream_t)stream, ws, g.n, g.t, tiles, keep_seq,
                     sums);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
