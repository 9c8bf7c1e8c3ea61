// Object-based verification: connected-component labelling of every frame, the per-object table, and SAL (Wernli et al. 2008,
// Mon. Wea. Rev. 136, 4470) of forecast / observation pairs.  Not in the reference.
//
// A frame is one (n, t) image of H x W pixels (C = 1), addressed in place through the element strides of its axes.  An object pixel
// is one with v >= thr and v > 0, thr = the caller's threshold or float(thr_factor) * max(frame) (ONE fp32 product: Wernli's
// R* = R_max / 15; a NaN in the frame makes that maximum NaN and the frame object-free, as numpy's max does).  Objects are the 4- or
// 8-connected components of that mask with at least min_pixels pixels, numbered 1, 2, ... in raster order of their first pixel.
//
// objects_label_kernel: one workgroup per frame, the label image lives in LDS as uint16 (row stride 128, any 1 <= H, W <= 128).
//   1. statistics: max, non-finite flags and the whole-field sums (sum v, sum v row, sum v col) in fp64: per-thread partials over a fixed
//      pixel set, wave butterflies, waves in order -- the same frame gives the same bits.
//   2. labelling by label equivalence: lab[p] = p on the mask, then (scan, compress) passes until a scan changes nothing.
//      scan:     m = the smallest label among p and its neighbours; where m < lab[p], lab[lab[p]] and lab[p] are lowered to m.
//      compress: lab[p] = the root of p's chain (r with lab[r] == r).
//      The stores of one phase race with its loads (plain 16-bit LDS stores, no atomics).  What holds regardless: every value ever stored
//      in lab[p] is the index of a pixel of p's component and is below the value the storing thread read from that cell, so at the end
//      of a phase every cell is <= its value at the phase's start; lab[p] <= p makes every chain strictly decreasing, so it ends at a
//      root.  TERMINATION: a scan that reports a change has lowered at least one cell and raised none, so the sum of the labels, a
//      non-negative integer, falls with every pass that goes on -- the loop ends, with no iteration cap.  THE RESULT IS UNIQUE: the
//      last scan stored nothing, so it read a consistent image in which no neighbour of any pixel has a smaller label, i.e. labels
//      are constant on components; the first pixel f of a component can only hold f (nothing of its component is smaller), so every
//      component carries the index of its first pixel whatever the races did.  Labels are therefore bit-reproducible.
//   3. min_pixels > 1: areas are counted per root (integer LDS atomics, batches of 8192 root indices) and small components dropped.
//   4. numbering: a prefix sum over the root flags in raster order gives the canonical ids; the label image becomes ids (0: background).
//   5. per-object sums, for any number of objects (8192 on a 4-connected 128 x 128 checkerboard): batches of 512 object slots in
//      LDS, one sweep over the pixels per batch.  A pixel's value is split into two 40-bit fixed-point limbs relative to the frame
//      maximum (hi = trunc(v 2^(40 - e)), lo = trunc of the exact remainder times 2^40, e: max < 2^e), which are added -- also times the
//      row and the column -- with INTEGER LDS atomics: the sums are exact for every pixel >= 2^-57 of the maximum (smaller ones are
//      truncated at 2^-80 of it), independent of the order of the additions, hence bit-reproducible although they use atomics; a wave
//      whose pixels all fall into one slot adds them up with shuffles first, which changes nothing for the same reason.  Peak: integer
//      max of the (positive) float bits.  The slots are converted to fp64 once: mass, peak, area, centroid -> table row; R^2 / P, R and
//      R |x - x_n| -> per-thread partials, slot s of every batch on thread s, folded in a fixed order at the end.
//   A frame with a non-finite pixel gets its labels and count, flag 1, and zero object sums (its pairs are skipped).
//
// sal_pair_kernel: (member record, target record) pairs -> the state sums, fp64, per-thread partials over a fixed pair set and a fixed
// tree: bit-reproducible for given records.  The target's frames are labelled once for all M members, in the members' launch (the
// grid's last N T workgroups read the second source): pd_sal_update is two launches.
#include "axes.h"
#include "common.h"

namespace {

constexpr int OB_THREADS = 512, OB_WAVES = OB_THREADS / 64;
constexpr int OB_MAX = 128;                     // the largest side
constexpr int OB_LOG = 7;                       // LDS row stride 128: cell = row << 7 | col
constexpr int OB_CELLS = OB_MAX * OB_MAX;
constexpr unsigned OB_BG = 0xFFFF, OB_DROP = 0xFFFE;   // >= OB_DROP: not an object pixel (the largest cell index is 16383)
constexpr int OB_AREA_BATCH = 8192;             // root indices per area-count batch (uint32 counters in the 32 KB aux buffer)
constexpr int OB_SLOTS = 512;                   // object slots per reduction batch
constexpr int OB_FX = 40;                       // bits per fixed-point limb
constexpr int OB_REC = 9;                       // doubles per frame record: D, sum v, sum v row, sum v col, V num, V den, r num, objects, flags
constexpr int OB_COLS = 6;                      // table row: mass, peak, area, row centroid, col centroid, first-pixel index
constexpr int OB_MAXM = 512;

struct ObSource {
  const float* base;
  int64_t s_lead, s_n, s_t, s_h, s_w;           // element strides: leading (member) axis, N, T, H, W
};

struct ObParams {
  int h, w;
  int64_t n, t;                                 // frames per leading index: n * t
  int64_t first_frames;                         // frames [0, first_frames) are the first source's, the rest the second's
  float thr, factor;
  int use_thr, conn8, min_pixels, max_objects;
};

// sum over the workgroup in a fixed order (called by every thread)
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double a = red[0];
#pragma unroll
  for (int i = 1; i < OB_WAVES; ++i) a += red[i];
  return a;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// two limbs -> fp64
__device__ __forceinline__ double fx_value(unsigned long long hi, unsigned long long lo, int e) {
  return ldexp((double)(long long)hi + ldexp((double)(long long)lo, -OB_FX), e - OB_FX);
}

__global__ void __launch_bounds__(OB_THREADS) objects_label_kernel(ObSource first, ObSource second, ObParams q,
                                                                   double* __restrict__ rec, int* __restrict__ labels,
                                                                   double* __restrict__ table) {
  __shared__ unsigned short lab_s[OB_CELLS];            // 32 KB: cell index while labelling, canonical id afterwards
  __shared__ unsigned long long aux[OB_CELLS / 4];      // 32 KB: area counters / ids of the roots / object slots
  __shared__ double red[OB_WAVES];
  __shared__ float fred[OB_WAVES];
  __shared__ int ired[OB_WAVES];
  volatile unsigned short* lab = lab_s;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = q.h, W = q.w, cells = H << OB_LOG;
  const int64_t f = blockIdx.x, per = q.n * q.t;
  const bool in_first = f < q.first_frames;
  const int64_t fl = in_first ? f : f - q.first_frames;
  const int64_t s_h = in_first ? first.s_h : second.s_h, s_w = in_first ? first.s_w : second.s_w;
  const float* __restrict__ src = (in_first ? first.base : second.base) + (fl / per) * (in_first ? first.s_lead : second.s_lead) +
                                  ((fl % per) / q.t) * (in_first ? first.s_n : second.s_n) + (fl % q.t) * (in_first ? first.s_t : second.s_t);

  // ---- 1. statistics
  float vmax = -INFINITY;
  int nonfinite = 0, isnan = 0;
  double sv = 0.0, svr = 0.0, svc = 0.0;
  for (int p = tid; p < cells; p += OB_THREADS) {
    const int r = p >> OB_LOG, c = p & (OB_MAX - 1);
    if (c >= W) continue;
    const float v = src[r * s_h + c * s_w];
    nonfinite |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    isnan |= v != v;
    vmax = fmaxf(vmax, v);
    const double dv = (double)v;
    sv += dv;
    svr = fma(dv, (double)r, svr);
    svc = fma(dv, (double)c, svc);
  }
  nonfinite = __syncthreads_or(nonfinite);
  isnan = __syncthreads_or(isnan);
  vmax = wave_max(vmax);
  if (lane == 0) fred[wave] = vmax;
  __syncthreads();
  vmax = fred[0];
#pragma unroll
  for (int i = 1; i < OB_WAVES; ++i) vmax = fmaxf(vmax, fred[i]);
  sv = block_sum(sv, red);
  svr = block_sum(svr, red);
  svc = block_sum(svc, red);
  float thr = q.use_thr ? q.thr : q.factor * vmax;
  if (!q.use_thr && isnan) thr = NAN;

  // ---- 2. labelling
  for (int p = tid; p < cells; p += OB_THREADS) {
    const int r = p >> OB_LOG, c = p & (OB_MAX - 1);
    bool obj = false;
    if (c < W) {
      const float v = src[r * s_h + c * s_w];
      obj = v >= thr && v > 0.0f;
    }
    lab[p] = obj ? (unsigned short)p : (unsigned short)OB_BG;
  }
  for (;;) {
    __syncthreads();
    int changed = 0;
    for (int p = tid; p < cells; p += OB_THREADS) {
      const unsigned l = lab[p];
      if (l >= OB_DROP) continue;
      const int r = p >> OB_LOG, c = p & (OB_MAX - 1);
      const bool w_ = c > 0, e_ = c + 1 < W, n_ = r > 0, s_ = r + 1 < H;
      unsigned m = l;
      if (w_) m = min(m, (unsigned)lab[p - 1]);
      if (e_) m = min(m, (unsigned)lab[p + 1]);
      if (n_) m = min(m, (unsigned)lab[p - OB_MAX]);
      if (s_) m = min(m, (unsigned)lab[p + OB_MAX]);
      if (q.conn8) {
        if (n_ && w_) m = min(m, (unsigned)lab[p - OB_MAX - 1]);
        if (n_ && e_) m = min(m, (unsigned)lab[p - OB_MAX + 1]);
        if (s_ && w_) m = min(m, (unsigned)lab[p + OB_MAX - 1]);
        if (s_ && e_) m = min(m, (unsigned)lab[p + OB_MAX + 1]);
      }
      if (m < l) {
        changed = 1;
        if (m < lab[l]) lab[l] = (unsigned short)m;
        if (m < lab[p]) lab[p] = (unsigned short)m;
      }
    }
    if (!__syncthreads_or(changed)) break;              // a scan that stored nothing: converged (see the header)
    for (int p = tid; p < cells; p += OB_THREADS) {
      const unsigned l = lab[p];
      if (l >= OB_DROP) continue;
      unsigned root = l, up;
      while ((up = lab[root]) != root) root = up;       // strictly decreasing: ends at a root
      if (root != l) lab[p] = (unsigned short)root;
    }
  }

  // ---- 3. components below min_pixels
  if (q.min_pixels > 1) {
    unsigned* cnt = (unsigned*)aux;
    for (int base = 0; base < cells; base += OB_AREA_BATCH) {
      for (int i = tid; i < OB_AREA_BATCH; i += OB_THREADS) cnt[i] = 0;
      __syncthreads();
      for (int p = tid; p < cells; p += OB_THREADS) {
        const unsigned l = lab[p];
        if (l < OB_DROP && l - (unsigned)base < (unsigned)OB_AREA_BATCH) atomicAdd(&cnt[l - base], 1u);
      }
      __syncthreads();
      const int end = min(base + OB_AREA_BATCH, cells);
      for (int p = base + tid; p < end; p += OB_THREADS)
        if (lab[p] == p && cnt[p - base] < (unsigned)q.min_pixels) lab[p] = (unsigned short)OB_DROP;
      __syncthreads();
    }
    // every label is a root's index, and this loop stores to no root's cell
    for (int p = tid; p < cells; p += OB_THREADS) {
      const unsigned l = lab[p];
      if (l < OB_DROP && l != (unsigned)p && lab[l] == OB_DROP) lab[p] = (unsigned short)OB_DROP;
    }
    __syncthreads();
  }

  // ---- 4. canonical ids: thread t numbers the roots of its run of consecutive cells after those of the threads before it
  unsigned short* ids = (unsigned short*)aux;
  const int chunk = (cells + OB_THREADS - 1) / OB_THREADS;
  const int p0 = min(tid * chunk, cells), p1 = min(p0 + chunk, cells);
  int mine = 0;
  for (int p = p0; p < p1; ++p) mine += lab[p] == p;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) ired[wave] = incl;
  __syncthreads();
  int before = 0, K = 0;
#pragma unroll
  for (int i = 0; i < OB_WAVES; ++i) {
    if (i < wave) before += ired[i];
    K += ired[i];
  }
  double* trow = table ? table + f * q.max_objects * OB_COLS : nullptr;
  int id = before + incl - mine;
  for (int p = p0; p < p1; ++p)
    if (lab[p] == p) {
      ids[p] = (unsigned short)++id;
      if (trow && id <= q.max_objects) trow[(id - 1) * OB_COLS + 5] = (double)((p >> OB_LOG) * W + (p & (OB_MAX - 1)));
    }
  __syncthreads();
  int* lout = labels ? labels + f * H * W : nullptr;
  for (int p = tid; p < cells; p += OB_THREADS) {
    const unsigned l = lab[p];
    const unsigned k = l < OB_DROP ? ids[l] : 0u;       // a cell is read by its own thread only; ids is not written here
    lab[p] = (unsigned short)k;
    const int r = p >> OB_LOG, c = p & (OB_MAX - 1);
    if (lout && c < W) lout[r * W + c] = (int)k;
  }
  __syncthreads();

  // ---- 5. per-object sums
  double a_vnum = 0.0, a_vden = 0.0, a_rnum = 0.0;
  if (K > 0 && !nonfinite) {
    int e;
    frexpf(vmax, &e);                                   // vmax < 2^e; every object pixel is in (0, vmax]
    const double X = svr / sv, Y = svc / sv;
    unsigned long long *mh = aux, *ml = aux + OB_SLOTS, *rh = aux + 2 * OB_SLOTS, *rl = aux + 3 * OB_SLOTS, *ch = aux + 4 * OB_SLOTS,
                       *cl = aux + 5 * OB_SLOTS;
    unsigned* pk = (unsigned*)(aux + 6 * OB_SLOTS);
    unsigned* ar = pk + OB_SLOTS;
    for (int b0 = 0; b0 < K; b0 += OB_SLOTS) {
      for (int i = tid; i < 7 * OB_SLOTS; i += OB_THREADS) aux[i] = 0ull;
      __syncthreads();
      for (int p = tid; p < cells; p += OB_THREADS) {   // whole waves run every iteration (cells is a multiple of 128)
        const int k = (int)lab[p] - 1 - b0;
        const bool in = k >= 0 && k < OB_SLOTS;
        const unsigned long long who = __ballot(in);
        if (!who) continue;
        const int r = p >> OB_LOG, c = p & (OB_MAX - 1);
        long long hi = 0, lo = 0;
        unsigned bits = 0;
        if (in) {
          const float v = src[r * s_h + c * s_w];
          bits = __float_as_uint(v);
          const double s = ldexp((double)v, OB_FX - e);               // < 2^40, exact
          hi = (long long)s;
          lo = (long long)ldexp(s - (double)hi, OB_FX);               // the remainder is exact
        }
        const int k0 = __shfl(k, __ffsll((long long)who) - 1, 64);
        const bool has_lo = __ballot(lo != 0) != 0ull;
        if (__ballot(in && k != k0) == 0ull) {                        // one slot for the whole wave: add up first
          const long long h = wave_sum_i64(hi), hr = wave_sum_i64(hi * r), hc = wave_sum_i64(hi * c);
          long long l = 0, lr = 0, lc = 0;
          if (has_lo) l = wave_sum_i64(lo), lr = wave_sum_i64(lo * r), lc = wave_sum_i64(lo * c);
          unsigned top = bits;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) top = max(top, (unsigned)__shfl_xor((int)top, o, 64));
          if (lane == 0) {
            atomicAdd(&mh[k0], (unsigned long long)h);
            atomicAdd(&rh[k0], (unsigned long long)hr);
            atomicAdd(&ch[k0], (unsigned long long)hc);
            if (has_lo) {
              atomicAdd(&ml[k0], (unsigned long long)l);
              atomicAdd(&rl[k0], (unsigned long long)lr);
              atomicAdd(&cl[k0], (unsigned long long)lc);
            }
            atomicMax(&pk[k0], top);
            atomicAdd(&ar[k0], (unsigned)__popcll(who));
          }
        } else if (in) {
          atomicAdd(&mh[k], (unsigned long long)hi);
          atomicAdd(&rh[k], (unsigned long long)(hi * r));
          atomicAdd(&ch[k], (unsigned long long)(hi * c));
          if (lo) {
            atomicAdd(&ml[k], (unsigned long long)lo);
            atomicAdd(&rl[k], (unsigned long long)(lo * r));
            atomicAdd(&cl[k], (unsigned long long)(lo * c));
          }
          atomicMax(&pk[k], bits);
          atomicAdd(&ar[k], 1u);
        }
      }
      __syncthreads();
      for (int s = tid; s < OB_SLOTS && b0 + s < K; s += OB_THREADS) {
        const double R = fx_value(mh[s], ml[s], e), P = (double)__uint_as_float(pk[s]);
        const double xr = fx_value(rh[s], rl[s], e) / R, xc = fx_value(ch[s], cl[s], e) / R;
        if (trow && b0 + s < q.max_objects) {
          double* row = trow + (b0 + s) * OB_COLS;
          row[0] = R, row[1] = P, row[2] = (double)ar[s], row[3] = xr, row[4] = xc;
        }
        a_vnum += R * (R / P);
        a_vden += R;
        if (sv != 0.0) a_rnum += R * sqrt((xr - X) * (xr - X) + (xc - Y) * (xc - Y));
      }
      __syncthreads();
    }
  }
  a_vnum = block_sum(a_vnum, red);
  a_vden = block_sum(a_vden, red);
  a_rnum = block_sum(a_rnum, red);
  if (tid == 0) {
    double* o = rec + f * OB_REC;
    o[0] = sv / ((double)H * (double)W), o[1] = sv, o[2] = svr, o[3] = svc;
    o[4] = a_vnum, o[5] = a_vden, o[6] = a_rnum, o[7] = (double)K, o[8] = nonfinite ? 1.0 : 0.0;
  }
}

// grid (T'): block tk folds the (member, n[, t]) pairs of its step.  rec: M N T member records, then N T target records.
// sums [7][T']: S, A, L1, L2, L, |S|, |A|;  counts [8][T']: pairs, skipped, S / A / L1 / L defined, objects in pred, in target.
__global__ void __launch_bounds__(256) sal_pair_kernel(const double* __restrict__ rec, int M, int64_t N, int64_t T, int keep_seq,
                                                       double diag, double* __restrict__ sums, long long* __restrict__ counts) {
  __shared__ double rs[256];
  __shared__ long long rc[256];
  const int tid = threadIdx.x, tk = blockIdx.x;
  const int64_t Tk = keep_seq ? T : 1;
  const int64_t total = keep_seq ? (int64_t)M * N : (int64_t)M * N * T;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = tid; i < total; i += 256) {
    int64_t m, n, t;
    if (keep_seq) m = i / N, n = i % N, t = tk;
    else m = i / (N * T), n = (i / T) % N, t = i % T;
    const double* F = rec + ((m * N + n) * T + t) * OB_REC;
    const double* O = rec + (((int64_t)M * N + n) * T + t) * OB_REC;
    if (F[8] != 0.0 || O[8] != 0.0) {
      c[1] += 1;
      continue;
    }
    c[0] += 1;
    c[6] += (long long)F[7];
    c[7] += (long long)O[7];
    const double dsum = F[0] + O[0];
    if (dsum != 0.0) {
      const double A = (F[0] - O[0]) / (0.5 * dsum);
      a[1] += A, a[6] += fabs(A), c[3] += 1;
    }
    const bool objs = F[7] > 0.0 && O[7] > 0.0, mass = F[1] != 0.0 && O[1] != 0.0 && diag > 0.0;
    if (objs) {
      const double VF = F[4] / F[5], VO = O[4] / O[5];
      const double S = (VF - VO) / (0.5 * (VF + VO));
      a[0] += S, a[5] += fabs(S), c[2] += 1;
    }
    if (mass) {
      const double dr = F[2] / F[1] - O[2] / O[1], dc = F[3] / F[1] - O[3] / O[1];
      const double L1 = sqrt(dr * dr + dc * dc) / diag;
      a[2] += L1, c[4] += 1;
      if (objs) {                                       // L2 needs the objects and the mass centre: L is defined where L2 is
        const double L2 = 2.0 * fabs(F[6] / F[5] - O[6] / O[5]) / diag;
        a[3] += L2, a[4] += L1 + L2, c[5] += 1;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    rs[tid] = a[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) rs[tid] += rs[tid + h];
      __syncthreads();
    }
    if (tid == 0) sums[k * Tk + tk] += rs[0];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    rc[tid] = c[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) rc[tid] += rc[tid + h];
      __syncthreads();
    }
    if (tid == 0) counts[k * Tk + tk] += rc[0];
    __syncthreads();
  }
}

// frames of a call with M leading members (M = 0: the frames of `sizes` alone); -1: unsupported
int64_t ob_frames(int M, const int64_t* sizes) {
  Axes5 g;
  if (M < 0 || M > OB_MAXM || !read_axes(sizes, g) || g.c != 1 || g.h > OB_MAX || g.w > OB_MAX) return -1;
  const double frames = (double)(M + 1) * (double)g.n * (double)g.t;
  return frames > (double)(1 << 30) ? -1 : (int64_t)(M + 1) * g.n * g.t;
}

int ob_check(const char* who, const int64_t* sizes, float thr_factor, int use_threshold, int connectivity, int min_pixels) {
  for (int i = 0; i < 5; ++i) PD_CHECK_ARG(sizes[i] >= 1, "%s: axis %d has size %lld", who, i, (long long)sizes[i]);
  PD_CHECK_ARG(sizes[4] == 1, "%s: C = %lld; objects are labelled on one channel", who, (long long)sizes[4]);
  PD_CHECK_ARG(sizes[2] <= OB_MAX && sizes[3] <= OB_MAX,
               "%s: %lld x %lld frames: the label image lives in LDS, sides up to %d are supported", who, (long long)sizes[2],
               (long long)sizes[3], OB_MAX);
  PD_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity %d (4 or 8)", who, connectivity);
  PD_CHECK_ARG(min_pixels >= 1, "%s: min_pixels = %d (>= 1)", who, min_pixels);
  PD_CHECK_ARG(use_threshold || thr_factor > 0.0f, "%s: thr_factor = %g (> 0)", who, (double)thr_factor);
  return PD_OK;
}

ObSource ob_source(const float* base, int64_t s_lead, const int64_t* strides) {
  return ObSource{base, s_lead, strides[0], strides[1], strides[2], strides[3]};
}

// one launch over the `lead` x N x T frames of `first` followed by the N x T frames of `second` (NULL: none); record f belongs to frame f
int ob_launch(ObSource first, int64_t lead, const ObSource* second, const int64_t* sizes, float threshold, int use_threshold,
              float thr_factor, int connectivity, int min_pixels, double* rec, int* labels, double* table, int max_objects,
              hipStream_t stream) {
  ObParams q;
  q.h = (int)sizes[2], q.w = (int)sizes[3], q.n = sizes[0], q.t = sizes[1];
  q.first_frames = lead * q.n * q.t;
  q.thr = threshold, q.factor = thr_factor, q.use_thr = use_threshold ? 1 : 0, q.conn8 = connectivity == 8;
  q.min_pixels = min_pixels, q.max_objects = max_objects;
  const int64_t frames = q.first_frames + (second ? q.n * q.t : 0);
  hipLaunchKernelGGL(objects_label_kernel, dim3((unsigned)frames), dim3(OB_THREADS), 0, stream, first, second ? *second : first, q, rec,
                     labels, table);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

}  // namespace

extern "C" int64_t pd_objects_ws_bytes(int M, const int64_t* sizes) {
  const int64_t frames = ob_frames(M, sizes);
  return frames < 0 ? -1 : frames * OB_REC * (int64_t)sizeof(double);
}

extern "C" int pd_objects_label(const float* frames, const int64_t* sizes, const int64_t* strides, float threshold, int use_threshold,
                                float thr_factor, int connectivity, int min_pixels, double* records, int* labels, double* table,
                                int max_objects, pd_stream_t stream) {
  PD_CHECK_ARG(frames && sizes && strides && records, "pd_objects_label: null pointer");
  if (int rc = ob_check("pd_objects_label", sizes, thr_factor, use_threshold, connectivity, min_pixels)) return rc;
  PD_CHECK_ARG(!table || max_objects >= 1, "pd_objects_label: a table of %d rows per frame", max_objects);
  PD_CHECK_ARG(ob_frames(0, sizes) > 0, "pd_objects_label: too many frames in one call");
  return ob_launch(ob_source(frames, 0, strides), 1, nullptr, sizes, threshold, use_threshold, thr_factor, connectivity, min_pixels,
                   records, labels, table, table ? max_objects : 0, (hipStream_t)stream);
}

extern "C" int pd_sal_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                             const int64_t* target_strides, float threshold, int use_threshold, float thr_factor, int connectivity,
                             int min_pixels, int keep_seq, double* sums, long long* counts, void* ws, int64_t ws_bytes,
                             pd_stream_t stream) {
  PD_CHECK_ARG(pred && target && sizes && pred_strides && target_strides && sums && counts && ws, "pd_sal_update: null pointer");
  PD_CHECK_ARG(M >= 1 && M <= OB_MAXM, "pd_sal_update: %d members (supported: 1 .. %d)", M, OB_MAXM);
  if (int rc = ob_check("pd_sal_update", sizes, thr_factor, use_threshold, connectivity, min_pixels)) return rc;
  const int64_t need = pd_objects_ws_bytes(M, sizes);
  PD_CHECK_ARG(need > 0, "pd_sal_update: too many frames in one update");
  PD_CHECK_ARG(ws_bytes >= need, "pd_sal_update: workspace of %lld bytes < %lld", (long long)ws_bytes, (long long)need);
  const int64_t N = sizes[0], T = sizes[1];
  double* rec = (double*)ws;
  const ObSource tsrc = ob_source(target, 0, target_strides);
  if (int rc = ob_launch(ob_source(pred, pred_strides[0], pred_strides + 1), M, &tsrc, sizes, threshold, use_threshold, thr_factor,
                         connectivity, min_pixels, rec, nullptr, nullptr, 0, (hipStream_t)stream))
    return rc;
  const double hh = (double)(sizes[2] - 1), ww = (double)(sizes[3] - 1);
  hipLaunchKernelGGL(sal_pair_kernel, dim3((unsigned)(keep_seq ? T : 1)), dim3(256), 0, (hipStream_t)stream, (const double*)rec, M, N, T,
                     keep_seq, sqrt(hh * hh + ww * ww), sums, counts);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
