// Frame scores of decoded samples against one target: squared error, absolute error and SSIM per lead time, read in place.
//
// What the reference's test_step gets from torchmetrics' MeanSquaredError, MeanAbsoluteError and (default)
// StructuralSimilarityIndexMeasure (scripts/prediff/sevirlr/train_sevirlr_prediff.py:937-965), in one launch instead of five stacked
// conv2d over a (5 B T, 1, H, W) tensor per sample.  pred holds M >= 1 members of target's shape; both are addressed through the
// element strides of their N, T, H, W, C axes (any layout, non-contiguous views), as pd_sevir_skill_counts_pooled does.
//
//   d = double(p) - double(t):  sum d^2 -> sums[0][t], sum |d| -> sums[1][t]                       (fp64: no fp32 summation order)
//   SSIM of one (n, t) frame (C channels of H x W): 11 x 11 Gaussian window, sigma 1.5, separable, weights summing to 1;
//     mu_p, mu_t, E[pp], E[tt], E[pt] the window means, var_p = max(E[pp] - mu_p^2, 0), var_t alike, cov = E[pt] - mu_p mu_t,
//     c1 = (0.01 R)^2, c2 = (0.03 R)^2, ssim = (2 mu_p mu_t + c1)(2 cov + c2) / ((mu_p^2 + mu_t^2 + c1)(var_p + var_t + c2)),
//     frame value = mean over the C (H - 10)(W - 10) windows that lie inside the frame                -> sums[2][t]
//   counts[0][t] += elements, counts[1][t] += frames.  No NaN masking: a NaN pixel makes its frame's SSIM and its step's sums NaN.
//
// One workgroup per 16 x 32 tile of window positions of one (n, t, c) plane.  The 26 x 42 input tile (tile + 10-pixel halo) of the
// target is staged in LDS once and its two moments (mu_t, E[tt]) are computed once and kept in registers; then, per member, the
// prediction's tile is staged, the horizontal 11-tap pass writes mu / E[pp] / E[pt] rows to LDS and the vertical pass reads them back:
// no intermediate reaches memory.  The pixels are fp32; every product and sum is fp64 (a product of two fp32 values is exact in
// fp64; about 150 fp64 FMAs per window position, ~1 GFLOP for 32 x 6 frames of 128 x 128), so var = E[xx] - mu^2 loses nothing to
// cancellation and the result needs no data-dependent centring.  Reduction: fixed-order wave butterflies, one partial
// triple per (member, tile) in the workspace, a fixed-order final pass per (step, sum) -- no floating-point atomics, the same inputs
// give the same bits.  data_range R is a host float, or max(range_buf[0], range_buf[1]) read on the device after frame_range_kernel
// has filled range_buf with max - min of pred and of target (torchmetrics' data_range=None); no value travels through the host.
#include "axes.h"
#include "common.h"

namespace {

constexpr int FS_THREADS = 256;
constexpr int FS_TAPS = 11, FS_HALO = FS_TAPS - 1;
constexpr int FS_TH = 16, FS_TW = 32;                          // window positions per tile
constexpr int FS_IH = FS_TH + FS_HALO, FS_IW = FS_TW + FS_HALO; // staged pixels per tile: 26 x 42
constexpr int FS_IWS = FS_IW + 1;                              // LDS row stride 43: two rows of a 32-lane group land on banks of both parities
constexpr int FS_MAXM = 512;
constexpr int FS_RANGE_BLOCKS = 256;                           // blocks of the min / max pass (5 partials each at the workspace's end)
constexpr int FS_RANGE_DOUBLES = FS_RANGE_BLOCKS * 5;

// exp(-d^2 / (2 * 1.5^2)), d = -5 .. 5, divided by their sum
__device__ const double FS_G[FS_TAPS] = {0.0010283800844791092, 0.007598758135239185, 0.03600077212843083, 0.10936068950970002,
                                         0.2130055377112537,    0.26601172486179436,  0.2130055377112537,  0.10936068950970002,
                                         0.03600077212843083,   0.007598758135239185, 0.0010283800844791092};

struct FsGeom : Axes5 {
  int ty, tx;                 // tiles per plane
};

// the 26 x 42 pixels at (r0, c0) of the plane at `src` -> dst (zero outside the frame: those feed no window that is counted)
__device__ __forceinline__ void stage_tile(const float* __restrict__ src, const Axes5& s, const FsGeom& g, int r0, int c0,
                                           float* __restrict__ dst) {
  for (int i = threadIdx.x; i < FS_IH * FS_IW; i += FS_THREADS) {
    const int lr = i / FS_IW, lc = i % FS_IW;
    const int64_t gr = r0 + lr, gc = c0 + lc;
    dst[lr * FS_IWS + lc] = gr < g.h && gc < g.w ? src[gr * s.h + gc * s.w] : 0.0f;
  }
}

// Horizontal pass.  Thread (row, cc) takes the window positions (row, 2 cc) and (row, 2 cc + 1) of rows tid / 16 and tid / 16 + 16:
// the 12 pixels they share are read once.  WITH_P: mu_p, E[pp], E[pt] -> hs[0..2]; otherwise mu_t, E[tt] -> hs[3..4].
template <bool WITH_P>
__device__ __forceinline__ void horizontal(const float* __restrict__ ps, const float* __restrict__ ts, double* __restrict__ hs) {
  const int cc = threadIdx.x % 16;
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int row = threadIdx.x / 16 + 16 * rr;
    if (row >= FS_IH) break;
    double a0[3] = {0.0, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k <= FS_TAPS; ++k) {
      const double t = (double)ts[row * FS_IWS + 2 * cc + k];
      double v0, v1, v2 = 0.0;
      if (WITH_P) {
        const double p = (double)ps[row * FS_IWS + 2 * cc + k];
        v0 = p, v1 = p * p, v2 = p * t;
      } else {
        v0 = t, v1 = t * t;
      }
      if (k < FS_TAPS) {
        a0[0] = fma(FS_G[k], v0, a0[0]);
        a0[1] = fma(FS_G[k], v1, a0[1]);
        if (WITH_P) a0[2] = fma(FS_G[k], v2, a0[2]);
      }
      if (k > 0) {
        a1[0] = fma(FS_G[k - 1], v0, a1[0]);
        a1[1] = fma(FS_G[k - 1], v1, a1[1]);
        if (WITH_P) a1[2] = fma(FS_G[k - 1], v2, a1[2]);
      }
    }
    constexpr int base = WITH_P ? 0 : 3, nm = WITH_P ? 3 : 2;
#pragma unroll
    for (int q = 0; q < nm; ++q) {
      hs[((base + q) * FS_IH + row) * FS_TW + 2 * cc] = a0[q];
      hs[((base + q) * FS_IH + row) * FS_TW + 2 * cc + 1] = a1[q];
    }
  }
}

// Vertical pass of moment q for the window positions (2 (tid / 32), tid % 32) and one row below: 12 rows of hs read once.
__device__ __forceinline__ void vertical(const double* __restrict__ hs, int q, double& o0, double& o1) {
  const int col = threadIdx.x % FS_TW, row0 = 2 * (threadIdx.x / FS_TW);
  double a0 = 0.0, a1 = 0.0;
#pragma unroll
  for (int k = 0; k <= FS_TAPS; ++k) {
    const double v = hs[(q * FS_IH + row0 + k) * FS_TW + col];
    if (k < FS_TAPS) a0 = fma(FS_G[k], v, a0);
    if (k > 0) a1 = fma(FS_G[k - 1], v, a1);
  }
  o0 = a0, o1 = a1;
}

// grid (planes * tiles, member chunks): block x = ((n T + t) C + c) tiles + tile scores members [y mchunk, (y + 1) mchunk) of its tile.
// ws[(m nwg + x) 3 + k]: sum d^2, sum |d| over the pixels the tile owns, and the sum of ssim over its window positions.
__global__ void __launch_bounds__(FS_THREADS) frame_score_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                 FsGeom g, int64_t pred_stride_m, Axes5 sp, Axes5 st, int M,
                                                                 int mchunk, float data_range, const float* __restrict__ range_buf,
                                                                 double* __restrict__ ws) {
  __shared__ float ps[FS_IH * FS_IWS], ts[FS_IH * FS_IWS];
  __shared__ double hs[5 * FS_IH * FS_TW];
  __shared__ double red[3][FS_THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t wg = blockIdx.x, nwg = gridDim.x;
  const int tiles = g.ty * g.tx;
  const int tile = (int)(wg % tiles);
  const int64_t plane = wg / tiles;
  const int64_t c = plane % g.c, t = (plane / g.c) % g.t, n = plane / (g.c * g.t);
  const int tyi = tile / g.tx, txi = tile % g.tx;
  const int r0 = tyi * FS_TH, c0 = txi * FS_TW;
  const int64_t hout = g.h - FS_HALO, wout = g.w - FS_HALO;

  float R = data_range;
  if (range_buf) {
    const float rp = range_buf[0], rt = range_buf[1];
    R = (rp != rp || rt != rt) ? NAN : fmaxf(rp, rt);
  }
  const double c1 = (0.01 * (double)R) * (0.01 * (double)R), c2 = (0.03 * (double)R) * (0.03 * (double)R);

  stage_tile(target + n * st.n + t * st.t + c * st.c, st, g, r0, c0, ts);
  __syncthreads();
  horizontal<false>(ps, ts, hs);
  __syncthreads();
  double mut[2], ett[2];
  vertical(hs, 3, mut[0], mut[1]);
  vertical(hs, 4, ett[0], ett[1]);

  // this thread's two window positions, and whether the frame has them
  const int ocol = tid % FS_TW, orow = 2 * (tid / FS_TW);
  const bool in0 = r0 + orow < hout && c0 + ocol < wout, in1 = r0 + orow + 1 < hout && c0 + ocol < wout;
  // the pixels this tile owns for the error sums: its 16 x 32 corner, plus the halo rows / columns in the last tile row / column
  const int own_h = tyi == g.ty - 1 ? FS_IH : FS_TH, own_w = txi == g.tx - 1 ? FS_IW : FS_TW;

  const int m1 = min(M, ((int)blockIdx.y + 1) * mchunk);
  for (int m = blockIdx.y * mchunk; m < m1; ++m) {
    __syncthreads();                                   // the last member's vertical pass and partials are done with hs / red
    stage_tile(pred + m * pred_stride_m + n * sp.n + t * sp.t + c * sp.c, sp, g, r0, c0, ps);
    __syncthreads();
    double sq = 0.0, ab = 0.0;
    for (int i = tid; i < FS_IH * FS_IW; i += FS_THREADS) {
      const int lr = i / FS_IW, lc = i % FS_IW;
      if (lr < own_h && lc < own_w && r0 + lr < g.h && c0 + lc < g.w) {
        const double d = (double)ps[lr * FS_IWS + lc] - (double)ts[lr * FS_IWS + lc];
        sq = fma(d, d, sq);
        ab += fabs(d);
      }
    }
    horizontal<true>(ps, ts, hs);
    __syncthreads();
    double mup[2], epp[2], ept[2];
    vertical(hs, 0, mup[0], mup[1]);
    vertical(hs, 1, epp[0], epp[1]);
    vertical(hs, 2, ept[0], ept[1]);
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double vp = fmax(epp[j] - mup[j] * mup[j], 0.0), vt = fmax(ett[j] - mut[j] * mut[j], 0.0);
      const double cov = ept[j] - mup[j] * mut[j];
      const double num = (2.0 * mup[j] * mut[j] + c1) * (2.0 * cov + c2);
      const double den = (mup[j] * mup[j] + mut[j] * mut[j] + c1) * (vp + vt + c2);
      // (fmax drops a NaN operand, but a NaN pixel is in mu as well -- every weight is nonzero -- so num is NaN with it)
      if (j == 0 ? in0 : in1) ss += num / den;
    }
    sq = wave_sum_f64(sq);
    ab = wave_sum_f64(ab);
    ss = wave_sum_f64(ss);
    if (lane == 0) {
      red[0][wave] = sq;
      red[1][wave] = ab;
      red[2][wave] = ss;
    }
    __syncthreads();
    if (tid < 3) ws[((int64_t)m * nwg + wg) * 3 + tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
  }
}

// grid (T', 3): sum k of step tk over its partials in a fixed order, added to sums[k][tk] (the ssim sums divided by the windows per
// frame: a frame's value is their mean); block (tk, 0) also adds the step's element and frame counts.
__global__ void __launch_bounds__(256) frame_score_final_kernel(const double* __restrict__ ws, FsGeom g, int M, int keep_seq,
                                                                double* __restrict__ sums, long long* __restrict__ counts) {
  __shared__ double r[256];
  const int tk = blockIdx.x, k = blockIdx.y;
  const int64_t Tk = keep_seq ? g.t : 1;
  const int64_t per = g.c * g.ty * g.tx, nwg = g.n * g.t * per;
  const int64_t total = keep_seq ? (int64_t)M * g.n * per : (int64_t)M * nwg;
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < total; i += 256) {
    int64_t b = i;
    if (keep_seq) {
      const int64_t m = i / (g.n * per), rem = i % (g.n * per);
      b = m * nwg + ((rem / per) * g.t + tk) * per + rem % per;
    }
    a += ws[b * 3 + k];
  }
  r[threadIdx.x] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) r[threadIdx.x] += r[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double v = k == 2 ? r[0] / (double)(g.c * (g.h - FS_HALO) * (g.w - FS_HALO)) : r[0];
    sums[k * Tk + tk] += v;
    if (k == 0) {                                      // the only writer of these two counters in this launch
      const int64_t frames = (int64_t)M * g.n * (keep_seq ? 1 : g.t);
      counts[tk] += frames * g.c * g.h * g.w;
      counts[Tk + tk] += frames;
    }
  }
}

// ------------------------------------------------------------------------------------------------------- data_range = None
// min / max of pred (M members) and of target.  A wave takes one (member | target, n, t, c, h) row at a time, its lanes the W axis.
// part[block][5]: min p, max p, min t, max t, NaN flags (bit 0: pred, bit 1: target).
__global__ void __launch_bounds__(256) frame_range_kernel(const float* __restrict__ pred, const float* __restrict__ target, FsGeom g,
                                                          int64_t pred_stride_m, Axes5 sp, Axes5 st, int M,
                                                          double* __restrict__ part) {
  __shared__ float red[4][4];
  __shared__ int nred[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = g.n * g.t * g.c * g.h, total = (int64_t)(M + 1) * rows;
  float mnp = INFINITY, mxp = -INFINITY, mnt = INFINITY, mxt = -INFINITY;
  int nan = 0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < total; row += (int64_t)gridDim.x * 4) {
    const int64_t m = row / rows, q = row % rows;
    const int64_t h = q % g.h, c = (q / g.h) % g.c, t = (q / (g.h * g.c)) % g.t, n = q / (g.h * g.c * g.t);
    const bool is_t = m == M;
    const Axes5& s = is_t ? st : sp;
    const float* src = is_t ? target + n * st.n + t * st.t + c * st.c + h * st.h
                            : pred + m * pred_stride_m + n * sp.n + t * sp.t + c * sp.c + h * sp.h;
    float lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    for (int64_t w = lane; w < g.w; w += 64) {
      const float v = src[w * s.w];
      bad |= v != v;
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
    if (is_t) mnt = fminf(mnt, lo), mxt = fmaxf(mxt, hi);
    else mnp = fminf(mnp, lo), mxp = fmaxf(mxp, hi);
    nan |= bad ? (is_t ? 2 : 1) : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mnp = fminf(mnp, __shfl_xor(mnp, o, 64));
    mxp = fmaxf(mxp, __shfl_xor(mxp, o, 64));
    mnt = fminf(mnt, __shfl_xor(mnt, o, 64));
    mxt = fmaxf(mxt, __shfl_xor(mxt, o, 64));
    nan |= __shfl_xor(nan, o, 64);
  }
  if (lane == 0) {
    red[0][wave] = mnp, red[1][wave] = mxp, red[2][wave] = mnt, red[3][wave] = mxt;
    nred[wave] = nan;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const int k = threadIdx.x;
    double v;
    if (k == 4) v = (double)(nred[0] | nred[1] | nred[2] | nred[3]);
    else if (k & 1) v = (double)fmaxf(fmaxf(red[k][0], red[k][1]), fmaxf(red[k][2], red[k][3]));
    else v = (double)fminf(fminf(red[k][0], red[k][1]), fminf(red[k][2], red[k][3]));
    part[(int64_t)blockIdx.x * 5 + k] = v;
  }
}

// one block: the partials of frame_range_kernel -> range_buf = [max p - min p, max t - min t] (NaN if the tensor holds one, as torch.max)
__global__ void __launch_bounds__(FS_RANGE_BLOCKS) frame_range_final_kernel(const double* __restrict__ part, int nblk,
                                                                            float* __restrict__ range_buf) {
  __shared__ float r[4][FS_RANGE_BLOCKS];
  __shared__ int nr[FS_RANGE_BLOCKS];
  const int tid = threadIdx.x;
  const bool on = tid < nblk;
  r[0][tid] = on ? (float)part[tid * 5 + 0] : INFINITY;
  r[1][tid] = on ? (float)part[tid * 5 + 1] : -INFINITY;
  r[2][tid] = on ? (float)part[tid * 5 + 2] : INFINITY;
  r[3][tid] = on ? (float)part[tid * 5 + 3] : -INFINITY;
  nr[tid] = on ? (int)part[tid * 5 + 4] : 0;
  __syncthreads();
  for (int h = FS_RANGE_BLOCKS / 2; h > 0; h >>= 1) {
    if (tid < h) {
      r[0][tid] = fminf(r[0][tid], r[0][tid + h]);
      r[1][tid] = fmaxf(r[1][tid], r[1][tid + h]);
      r[2][tid] = fminf(r[2][tid], r[2][tid + h]);
      r[3][tid] = fmaxf(r[3][tid], r[3][tid + h]);
      nr[tid] |= nr[tid + h];
    }
    __syncthreads();
  }
  if (tid < 2) range_buf[tid] = (nr[0] >> tid) & 1 ? NAN : r[2 * tid + 1][0] - r[2 * tid][0];
}

bool fs_geom(const int64_t* sizes, FsGeom& g) {
  if (!read_axes(sizes, g)) return false;
  if (g.h < FS_TAPS || g.w < FS_TAPS || g.h > (1 << 20) || g.w > (1 << 20)) return false;
  g.ty = (int)((g.h - FS_HALO + FS_TH - 1) / FS_TH);
  g.tx = (int)((g.w - FS_HALO + FS_TW - 1) / FS_TW);
  return true;
}

// workgroups of one member; -1 when the grid or the element count would not fit
int64_t fs_nwg(const FsGeom& g) {
  const double planes = (double)g.n * (double)g.t * (double)g.c;
  if (planes * g.ty * g.tx >= (double)(1 << 30) || planes * (double)g.h * (double)g.w >= (double)(1ll << 40)) return -1;
  return g.n * g.t * g.c * g.ty * g.tx;
}

}  // namespace

extern "C" int64_t pd_frame_score_ws_doubles(int M, const int64_t* sizes) {
  FsGeom g;
  if (M < 1 || M > FS_MAXM || !fs_geom(sizes, g)) return -1;
  const int64_t nwg = fs_nwg(g);
  if (nwg < 0 || (double)nwg * M >= (double)(1ll << 34)) return -1;
  return nwg * M * 3 + FS_RANGE_DOUBLES;
}

extern "C" int pd_frame_score_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                                     const int64_t* target_strides, float data_range, float* range_buf, int keep_seq, double* sums,
                                     long long* counts, double* ws, int64_t ws_doubles, pd_stream_t stream) {
  PD_CHECK_ARG(pred && target && sizes && pred_strides && target_strides && sums && counts && ws, "pd_frame_score_update: null pointer");
  PD_CHECK_ARG(M >= 1 && M <= FS_MAXM, "pd_frame_score_update: %d members (supported: 1 .. %d)", M, FS_MAXM);
  for (int i = 0; i < 5; ++i) PD_CHECK_ARG(sizes[i] >= 1, "pd_frame_score_update: axis %d has size %lld", i, (long long)sizes[i]);
  PD_CHECK_ARG(sizes[2] >= FS_TAPS && sizes[3] >= FS_TAPS,
               "pd_frame_score_update: %lld x %lld frames hold no 11 x 11 SSIM window (H and W must be >= 11)", (long long)sizes[2],
               (long long)sizes[3]);
  FsGeom g;
  const int64_t need = pd_frame_score_ws_doubles(M, sizes);
  PD_CHECK_ARG(fs_geom(sizes, g) && need > 0, "pd_frame_score_update: too many frames / pixels in one update");
  PD_CHECK_ARG(ws_doubles >= need, "pd_frame_score_update: workspace of %lld doubles < %lld", (long long)ws_doubles, (long long)need);
  const int64_t nwg = fs_nwg(g);
  const Axes5 sp = read_strides(pred_strides + 1), st = read_strides(target_strides);
  if (range_buf) {
    double* part = ws + nwg * M * 3;
    const int64_t rows = (int64_t)(M + 1) * g.n * g.t * g.c * g.h;
    const int nblk = (int)std::min<int64_t>(FS_RANGE_BLOCKS, (rows + 3) / 4);
    hipLaunchKernelGGL(frame_range_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, pred, target, g, pred_strides[0], sp, st, M,
                       part);
    PD_CHECK_LAUNCH();
    hipLaunchKernelGGL(frame_range_final_kernel, dim3(1), dim3(FS_RANGE_BLOCKS), 0, (hipStream_t)stream, part, nblk, range_buf);
    PD_CHECK_LAUNCH();
  }
  // members per workgroup: all of them (the target's tile and moments are computed once), halved while the grid has fewer than 1024
  // workgroups and a workgroup still serves at least 4 members.  The partials are indexed by member: the fold order does not change.
  int mchunk = M;
  while (mchunk > 4 && nwg * ((M + mchunk - 1) / mchunk) < 1024) mchunk = (mchunk + 1) / 2;
  const int chunks = (M + mchunk - 1) / mchunk;
  hipLaunchKernelGGL(frame_score_kernel, dim3((unsigned)nwg, (unsigned)chunks), dim3(FS_THREADS), 0, (hipStream_t)stream, pred, target, g,
                     pred_strides[0], sp, st, M, mchunk, data_range, (const float*)range_buf, ws);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(frame_score_final_kernel, dim3((unsigned)(keep_seq ? g.t : 1), 3), dim3(256), 0, (hipStream_t)stream,
                     (const double*)ws, g, M, keep_seq, sums, counts);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
