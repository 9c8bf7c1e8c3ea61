// Optical-flow extrapolation (Lagrangian persistence; DESIGN.md §7 "Extrapolation baseline", prediff_amd/extrapolation.py, whose module
// docstring is the definition): pyramidal, iterated, damped Lucas-Kanade motion of a context, and semi-Lagrangian advection of its last
// frame.  fp32 throughout, no 16-bit operands (one build, no pd_call_opts), no atomics: the same input gives the same bits.
//
//   pd_lk_motion: levels - 1 launches of lk_down_kernel (the P + 1 newest frames of every sequence, one level each), then
//   levels * iters launches of lk_iter_kernel, coarsest level first.  Level 0 is read from the context in place.
//   pd_advect: one launch for all K frames of all B sequences.
//
// lk_iter_kernel, one iteration of one level.  A workgroup of 1024 threads owns a 32 x 32 output tile of one sequence; with R = radius its
// region is the (32 + 2 R)^2 cells whose products the tile's windows sum.  Per pair p (ascending):
//   stage   I0_p over the region plus one cell (the gradients' taps), coordinates clamped to the frame, so that a staged neighbour IS the
//           replicate border;
//   gather  per region cell inside the frame: the four clamped taps of the warped I1_p from global memory (the pyramid is L2-resident), at
//           the flow there (the source buffer; in the first iteration of a level twice the coarser level's cell -- the transfer is folded
//           in, no upsampled field exists; read once, the sample positions serve every pair), then the five products gy gy, gy gx,
//           gx gx, gy It, gx It, added to five LDS fields (one owner per cell, p ascending).  Cells outside the frame hold zeros: the
//           truncated box.  A thread's loads of a pair -- 3 staged cells, 12 taps -- are issued together.
// Then the separable box sums in LDS: along x every thread sums its (field, row, column) items into registers, a barrier, and the sums go
// back over the same fields with a pitch of 32 (in place: 5 fields and the staging tile are all the LDS there is, 51.5 KB at R = 7);
// along y every thread sums the five fields of its output cell, solves the damped 2 x 2 system and writes v - d.  G is recomputed in
// every iteration, never stored.  Source and destination flow buffers differ (a workgroup reads its neighbours' cells), the last
// iteration of level 0 writes the caller's tensor.  1024 threads: a workgroup's time is its own instruction stream, which four waves
// per SIMD share.
// Bank conflicts: consecutive lanes read consecutive columns everywhere (staging, products, both box passes): conflict-free.
// Every index is formed from clamped integers or from a float clamped to the frame first (a NaN clamps to 0): garbage in the context gives
// garbage motion, never an address outside the buffers.
#include "bilinear.h"
#include "common.h"

namespace {

constexpr int LK_THREADS = 1024;
constexpr int LK_TILE = 32;
constexpr int LK_MAX_RADIUS = 9;                               // (34 + 2 R)^2 + 5 (32 + 2 R)^2 floats <= 64 KiB
constexpr int LK_RSTEP = LK_THREADS / LK_TILE;                 // rows a pass of all threads covers, a thread to a column
constexpr int LK_HSUMS = 8;                                    // row sums a thread holds: 5 (32 + 2 R) <= 8 LK_RSTEP
constexpr int LK_CELLS = 3, LK_BATCH = 3, LK_STAGE = 3;        // region / staged cells of a thread: (32 + 2 R)^2, (34 + 2 R)^2 <= 3 LK_THREADS
constexpr int LK_MAX_SIDE = 512, LK_MIN_COARSE = 4, LK_MAX_LEVELS = 8, LK_MAX_PAIRS = 16, LK_MAX_ITERS = 64;
constexpr int LK_MAX_RW = LK_TILE + 2 * LK_MAX_RADIUS;
static_assert(LK_MAX_RW * LK_MAX_RW <= LK_CELLS * LK_THREADS && (LK_MAX_RW + 2) * (LK_MAX_RW + 2) <= LK_STAGE * LK_THREADS &&
              5 * LK_MAX_RW <= LK_HSUMS * LK_RSTEP && LK_CELLS % LK_BATCH == 0 && LK_TILE % LK_RSTEP == 0,
              "a thread's share of the region, the staged tile and the row sums at the largest radius");
static_assert(((LK_MAX_RW + 2) * (LK_MAX_RW + 2) + 5 * LK_MAX_RW * LK_MAX_RW) * 4 <= 64 * 1024, "LDS at the largest radius");

struct LkGeom {
  int P, levels;
  int h[LK_MAX_LEVELS], w[LK_MAX_LEVELS];
  int64_t pyr_off[LK_MAX_LEVELS], flow_off[LK_MAX_LEVELS][2];  // float offsets into the workspace (pyr_off[0] unused)
  int64_t floats;
};

bool lk_geom(int64_t B, int T, int H, int W, int levels, int iters, int radius, int pairs, LkGeom& g) {
  if (B < 1 || B > (1 << 20) || T < 2 || T > (1 << 16) || levels < 1 || levels > LK_MAX_LEVELS || iters < 1 || iters > LK_MAX_ITERS ||
      radius < 1 || radius > LK_MAX_RADIUS || pairs < 1)
    return false;
  if (H < 1 || W < 1 || H > LK_MAX_SIDE || W > LK_MAX_SIDE) return false;
  const int f = 1 << (levels - 1);
  if (H % f || W % f || H / f < LK_MIN_COARSE || W / f < LK_MIN_COARSE) return false;
  g.P = pairs < T - 1 ? pairs : T - 1;
  if (g.P > LK_MAX_PAIRS) return false;
  g.levels = levels;
  int64_t off = 0;
  for (int l = 0; l < levels; ++l) {
    g.h[l] = H >> l, g.w[l] = W >> l;
    const int64_t hw = (int64_t)g.h[l] * g.w[l];
    g.pyr_off[l] = off;
    if (l > 0) off += B * (g.P + 1) * hw;
    for (int k = 0; k < 2; ++k) g.flow_off[l][k] = off, off += B * 2 * hw;
  }
  g.floats = off;
  return true;
}

// level l + 1 from level l: the mean of each 2 x 2 block, ((a + b) + (c + d)) / 4.  One thread per destination cell, x fastest.
__global__ void __launch_bounds__(256) lk_down_kernel(const float* __restrict__ src, int64_t src_seq_stride, float* __restrict__ dst, int nf,
                                                      int Hd, int Wd, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % Wd);
  const int64_t q = i / Wd;
  const int y = (int)(q % Hd);
  const int64_t bf = q / Hd;
  const int f = (int)(bf % nf);
  const int64_t b = bf / nf;
  const float* s = src + b * src_seq_stride + (int64_t)f * (4 * Hd * Wd) + (int64_t)(2 * y) * (2 * Wd) + 2 * x;
  const float a = s[0], bb = s[1], c = s[2 * Wd], d = s[2 * Wd + 1];
  dst[i] = ((a + bb) + (c + d)) * 0.25f;
}

enum { LK_FLOW_ZERO = 0, LK_FLOW_COARSE = 1, LK_FLOW_SAME = 2 };

// the flow of cell (y, x) of this level before the iteration: 0, twice the coarser level's cell (y / 2, x / 2), or the source buffer's
__device__ __forceinline__ void lk_flow_at(const float* __restrict__ vsrc, int mode, int H, int W, int y, int x, float& vy, float& vx) {
  if (mode == LK_FLOW_ZERO) {
    vy = 0.f, vx = 0.f;
  } else if (mode == LK_FLOW_COARSE) {
    const int Hc = H >> 1, Wc = W >> 1;
    const int o = (y >> 1) * Wc + (x >> 1);
    vy = 2.f * vsrc[o], vx = 2.f * vsrc[Hc * Wc + o];
  } else {
    vy = vsrc[y * W + x], vx = vsrc[H * W + y * W + x];
  }
}

// grid: tiles_x * tiles_y * B workgroups, tile column fastest.  frames: frame 0 of the pyramid of sequence 0 at this level (frame f is
// ctx[:, T - 1 - P + f]); vsrc / vdst: [B][2][.][.] (vsrc at the coarser level's size when mode = LK_FLOW_COARSE).
__global__ void __launch_bounds__(LK_THREADS) lk_iter_kernel(const float* __restrict__ frames, int64_t seq_stride, int P, int H, int W,
                                                             const float* __restrict__ vsrc, int mode, float* __restrict__ vdst, int R,
                                                             float lam, int tiles_x, int tiles_y) {
  extern __shared__ __attribute__((aligned(16))) float lk_lds[];
  const int tid = threadIdx.x;
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y;
  const int64_t b = blockIdx.x / tiles_x / tiles_y;
  const int RW = LK_TILE + 2 * R, SW = RW + 2;                 // region side, staged side
  const int y00 = ty * LK_TILE - R, x00 = tx * LK_TILE - R;     // frame coordinates of region cell (0, 0)
  float* stage = lk_lds;                                       // [SW][SW]
  float* fld = lk_lds + SW * SW;                               // [5][RW][RW], then [5][RW][32]
  const int rcells = RW * RW;
  const int HW = H * W;
  const float* __restrict__ seq = frames + b * seq_stride;
  const int64_t vsrc_seq = mode == LK_FLOW_COARSE ? 2 * (int64_t)(H >> 1) * (W >> 1) : 2 * (int64_t)HW;
  const float* __restrict__ vs = mode == LK_FLOW_ZERO ? vsrc : vsrc + b * vsrc_seq;

  // What is the same for every pair, once: where this thread's staged cells come from, and per region cell of the thread
  // (cell = tid + k * LK_THREADS) the place of its gradient taps in the staged tile and of the warped I1 sample in the frame.  All loops over a
  // thread's cells have compile-time bounds and are unrolled: the loads of all cells are in flight together, nothing is indexed at run time.
  int soff[LK_STAGE];                                          // frame offset of staged cell tid + k * LK_THREADS, -1 beyond the tile
#pragma unroll
  for (int k = 0; k < LK_STAGE; ++k) {
    const int i = tid + k * LK_THREADS;
    const int sy = i / SW, sx = i - sy * SW;
    const int y = min(max(y00 - 1 + sy, 0), H - 1), x = min(max(x00 - 1 + sx, 0), W - 1);
    soff[k] = i < SW * SW ? y * W + x : -1;
  }
  int spos[LK_CELLS], tap[LK_CELLS];                           // staged index of the cell; y0 << 16 | x0 of the sample, -1: not in the frame
  float fy[LK_CELLS], fx[LK_CELLS];
#pragma unroll
  for (int k = 0; k < LK_CELLS; ++k) {
    const int i = tid + k * LK_THREADS;
    const int ry = i / RW, rx = i - ry * RW;
    const int y = y00 + ry, x = x00 + rx;
    spos[k] = (ry + 1) * SW + rx + 1, tap[k] = -1, fy[k] = 0.f, fx[k] = 0.f;
    if (i < rcells) {
      if (y >= 0 && y < H && x >= 0 && x < W) {
        float vy, vx;
        lk_flow_at(vs, mode, H, W, y, x, vy, vx);
        const float cy = fminf(fmaxf((float)y + vy, 0.f), (float)(H - 1));      // fmaxf(NaN, 0) = 0
        const float cx = fminf(fmaxf((float)x + vx, 0.f), (float)(W - 1));
        const float y0f = floorf(cy), x0f = floorf(cx);
        fy[k] = cy - y0f, fx[k] = cx - x0f;
        tap[k] = ((int)y0f << 16) | (int)x0f;
      } else {
#pragma unroll
        for (int f = 0; f < 5; ++f) fld[f * rcells + i] = 0.f;
      }
    }
  }

  for (int p = 0; p < P; ++p) {
    const float* __restrict__ I0 = seq + (int64_t)(P - 1 - p) * HW;
    const float* __restrict__ I1 = seq + (int64_t)(P - p) * HW;
    float sv[LK_STAGE];
#pragma unroll
    for (int k = 0; k < LK_STAGE; ++k) sv[k] = soff[k] >= 0 ? I0[soff[k]] : 0.f;
    if (p) __syncthreads();                                    // the products of pair p - 1 have read the staged tile
#pragma unroll
    for (int k = 0; k < LK_STAGE; ++k)
      if (soff[k] >= 0) stage[tid + k * LK_THREADS] = sv[k];
    __syncthreads();
#pragma unroll
    for (int h = 0; h < LK_CELLS; h += LK_BATCH) {             // LK_BATCH cells at a time: their 4 LK_BATCH taps are in flight together
      float t00[LK_BATCH], t01[LK_BATCH], t10[LK_BATCH], t11[LK_BATCH];
#pragma unroll
      for (int j = 0; j < LK_BATCH; ++j) {                     // bilinear from floor, the upper taps clamped too
        const int k = h + j;
        t00[j] = t01[j] = t10[j] = t11[j] = 0.f;
        if (tap[k] >= 0) {
          const int y0 = tap[k] >> 16, x0 = tap[k] & 0xffff;
          const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
          t00[j] = I1[y0 * W + x0], t01[j] = I1[y0 * W + x1], t10[j] = I1[y1 * W + x0], t11[j] = I1[y1 * W + x1];
        }
      }
#pragma unroll
      for (int j = 0; j < LK_BATCH; ++j) {
        const int k = h + j;
        if (tap[k] < 0) continue;
        const int i = tid + k * LK_THREADS;
        const float* c = stage + spos[k];
        const float gy = (c[SW] - c[-SW]) * 0.5f, gx = (c[1] - c[-1]) * 0.5f;
        const float top = t00[j] + fx[k] * (t01[j] - t00[j]);
        const float bot = t10[j] + fx[k] * (t11[j] - t10[j]);
        const float it = top + fy[k] * (bot - top) - c[0];
        const float q[5] = {gy * gy, gy * gx, gx * gx, gy * it, gx * it};
#pragma unroll
        for (int f = 0; f < 5; ++f) fld[f * rcells + i] = p ? fld[f * rcells + i] + q[f] : q[f];
      }
    }
  }
  __syncthreads();

  // along x: the sum of (field, region row) q and column c lands at fld[q * 32 + c]
  // (item k of a thread is row (tid >> 5) + LK_RSTEP k of the 5 RW (field, region row) rows, column tid & 31).  The tap loop is the outer one
  // in both passes: its unrolled body reads one tap of every sum of the thread, all independent, so the LDS latency is paid once per tap
  // and not once per tap and sum; each sum still adds its taps in ascending order.
  const int rows = 5 * RW, taps = 2 * R + 1;
  const int ox = tid & 31, row0 = tid >> 5;
  float hs[LK_HSUMS];
#pragma unroll
  for (int k = 0; k < LK_HSUMS; ++k) hs[k] = fld[min(row0 + LK_RSTEP * k, rows - 1) * RW + ox];     // rows beyond the last: read in bounds, not written
  for (int j = 1; j < taps; ++j) {
#pragma unroll
    for (int k = 0; k < LK_HSUMS; ++k) hs[k] += fld[min(row0 + LK_RSTEP * k, rows - 1) * RW + ox + j];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < LK_HSUMS; ++k)
    if (row0 + LK_RSTEP * k < rows) fld[(row0 + LK_RSTEP * k) * LK_TILE + ox] = hs[k];
  __syncthreads();

  // along y, the solve and the update: LK_TILE / LK_RSTEP output cells per thread
  const int x = tx * LK_TILE + ox;
  float s[LK_TILE / LK_RSTEP][5];
#pragma unroll
  for (int k = 0; k < LK_TILE / LK_RSTEP; ++k)
#pragma unroll
    for (int f = 0; f < 5; ++f) s[k][f] = fld[(f * RW + row0 + LK_RSTEP * k) * LK_TILE + ox];
  for (int j = 1; j < taps; ++j) {
#pragma unroll
    for (int k = 0; k < LK_TILE / LK_RSTEP; ++k)
#pragma unroll
      for (int f = 0; f < 5; ++f) s[k][f] += fld[(f * RW + row0 + LK_RSTEP * k + j) * LK_TILE + ox];
  }
#pragma unroll
  for (int k = 0; k < LK_TILE / LK_RSTEP; ++k) {
    const int y = ty * LK_TILE + row0 + LK_RSTEP * k;
    if (y >= H || x >= W) continue;
    const float a = s[k][0] + lam, c = s[k][2] + lam, g = s[k][1];
    const float det = a * c - g * g;
    const float dy = (c * s[k][3] - g * s[k][4]) / det, dx = (a * s[k][4] - g * s[k][3]) / det;
    float vy, vx;
    lk_flow_at(vs, mode, H, W, y, x, vy, vx);
    float* out = vdst + b * 2 * (int64_t)HW + y * W + x;
    out[0] = vy - dy;
    out[HW] = vx - dx;
  }
}

// F_k(y, x) = bil_fill(frame, y - k v_y, x - k v_x) (bilinear.h), k = 1 .. K: one thread per (b, y, x), x fastest, so that each of its K
// stores is coalesced along W.
__global__ void __launch_bounds__(256) advect_kernel(const float* __restrict__ frame, int64_t frame_stride, const float* __restrict__ motion,
                                                     float* __restrict__ out, int K, int H, int W, int64_t total, float fill) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int HW = H * W;
  const int64_t b = i / HW;
  const int yx = (int)(i - b * HW);
  const int y = yx / W, x = yx - y * W;
  const float* __restrict__ I = frame + b * frame_stride;
  const float vy = motion[b * 2 * (int64_t)HW + yx], vx = motion[b * 2 * (int64_t)HW + HW + yx];
  float* o = out + b * K * (int64_t)HW + yx;
#pragma unroll 4
  for (int k = 1; k <= K; ++k, o += HW) {
    *o = bil_fill(I, H, W, (float)y - (float)k * vy, (float)x - (float)k * vx, fill);
  }
}

}  // namespace

extern "C" int64_t pd_lk_ws_bytes(int64_t B, int T, int H, int W, int levels, int iters, int radius, int pairs) {
  LkGeom g;
  if (!lk_geom(B, T, H, W, levels, iters, radius, pairs, g)) return -1;
  return g.floats * 4;
}

extern "C" int pd_lk_motion(const float* ctx, float* motion, int64_t B, int T, int H, int W, int levels, int iters, int radius, float damping,
                            int pairs, void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(ctx && motion && ws, "pd_lk_motion: null pointer");
  LkGeom g;
  PD_CHECK_ARG(lk_geom(B, T, H, W, levels, iters, radius, pairs, g),
               "pd_lk_motion: unsupported shape or options (ctx (%lld, %d, %d, %d, 1), levels=%d iters=%d radius=%d pairs=%d): T >= 2, sides "
               "<= %d and divisible by 2^(levels - 1) with a coarsest side >= %d, 1 <= radius <= %d, min(pairs, T - 1) <= %d",
               (long long)B, T, H, W, levels, iters, radius, pairs, LK_MAX_SIDE, LK_MIN_COARSE, LK_MAX_RADIUS, LK_MAX_PAIRS);
  PD_CHECK_ARG(damping > 0.f && damping < INFINITY, "pd_lk_motion: damping must be positive and finite (the 2 x 2 system is solved in closed form)");
  PD_CHECK_ARG(ws_bytes >= g.floats * 4 && ((uintptr_t)ws & 3) == 0, "pd_lk_motion: the workspace holds %lld bytes, %lld are needed",
               (long long)ws_bytes, (long long)g.floats * 4);
  float* w = (float*)ws;
  const int nf = g.P + 1;
  const int64_t HW = (int64_t)H * W;
  const hipStream_t st = (hipStream_t)stream;

  for (int l = 1; l < levels; ++l) {
    const float* src = l == 1 ? ctx + (int64_t)(T - 1 - g.P) * HW : w + g.pyr_off[l - 1];
    const int64_t src_seq = l == 1 ? (int64_t)T * HW : (int64_t)nf * g.h[l - 1] * g.w[l - 1];
    const int64_t total = B * nf * g.h[l] * g.w[l];
    PD_CHECK_ARG((total + 255) / 256 <= 0x7fffffff, "pd_lk_motion: %lld pyramid cells at level %d", (long long)total, l);
    hipLaunchKernelGGL(lk_down_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, src_seq, w + g.pyr_off[l], nf, g.h[l],
                       g.w[l], total);
    PD_CHECK_LAUNCH();
  }

  const int RW = LK_TILE + 2 * radius;
  const int lds = ((RW + 2) * (RW + 2) + 5 * RW * RW) * 4;
  if (lds > 48 * 1024) {
    static bool attr_set_dev[PD_MAX_DEVICES];
    if (int rc = pd_raise_lds("pd_lk_motion", (const void*)lk_iter_kernel, 64 * 1024, attr_set_dev)) return rc;
  }
  const float* prev = w;                                       // never read in the first launch (LK_FLOW_ZERO)
  for (int l = levels - 1; l >= 0; --l) {
    const float* fr = l == 0 ? ctx + (int64_t)(T - 1 - g.P) * HW : w + g.pyr_off[l];
    const int64_t seq = l == 0 ? (int64_t)T * HW : (int64_t)nf * g.h[l] * g.w[l];
    const int tiles_x = (g.w[l] + LK_TILE - 1) / LK_TILE, tiles_y = (g.h[l] + LK_TILE - 1) / LK_TILE;
    const int64_t grid = (int64_t)tiles_x * tiles_y * B;
    PD_CHECK_ARG(grid <= 0x7fffffff, "pd_lk_motion: %lld workgroups", (long long)grid);
    for (int it = 0; it < iters; ++it) {
      const int mode = it ? LK_FLOW_SAME : l == levels - 1 ? LK_FLOW_ZERO : LK_FLOW_COARSE;
      float* dst = l == 0 && it == iters - 1 ? motion : w + g.flow_off[l][it & 1];
      hipLaunchKernelGGL(lk_iter_kernel, dim3((unsigned)grid), dim3(LK_THREADS), (size_t)lds, st, fr, seq, g.P, g.h[l], g.w[l], prev, mode,
                         dst, radius, damping, tiles_x, tiles_y);
      PD_CHECK_LAUNCH();
      prev = dst;
    }
  }
  return PD_OK;
}

extern "C" int pd_advect(const float* frame, const float* motion, float* out, int64_t B, int K, int H, int W, int64_t frame_stride,
                         float fill, pd_stream_t stream) {
  PD_CHECK_ARG(frame && motion && out && B > 0 && K > 0 && H > 0 && W > 0, "pd_advect: bad args (frame (%lld, %d, %d), K=%d)", (long long)B,
               H, W, K);
  PD_CHECK_ARG(H <= LK_MAX_SIDE && W <= LK_MAX_SIDE && B <= (1 << 20) && K <= (1 << 12), "pd_advect: frame (%lld, %d, %d), K=%d: sides <= %d",
               (long long)B, H, W, K, LK_MAX_SIDE);
  PD_CHECK_ARG(frame_stride >= (int64_t)H * W, "pd_advect: frame_stride %lld is below one frame", (long long)frame_stride);
  PD_CHECK_ARG(fill == fill && fill - fill == 0.f, "pd_advect: fill must be finite");
  PD_CHECK_ARG((const void*)out != (const void*)frame && (const void*)out != (const void*)motion, "pd_advect: out aliases an input");
  const int64_t total = B * H * W;
  PD_CHECK_ARG((total + 255) / 256 <= 0x7fffffff, "pd_advect: %lld cells", (long long)total);
  hipLaunchKernelGGL(advect_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, frame, frame_stride, motion, out,
                     K, H, W, total, fill);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
