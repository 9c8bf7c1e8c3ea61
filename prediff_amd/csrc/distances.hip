// Distance-map verification: the exact squared Euclidean distance transform of the event set of every frame, and the mean error
// distances, the Hausdorff distance and Baddeley's Delta of forecast / observation pairs (Gilleland 2011, 2017).  Not in the reference.
//
// A frame is one (n, t) image of H x W pixels (C = 1, 1 <= H, W <= 128), addressed in place through the element strides of its axes.
// Event set of threshold k: { s : v[s] / divisor >= thr_k } -- the IEEE division and comparison of pd_sevir_skill_counts; a NaN is never
// an event.  d2[s] = min over events a of (row_s - row_a)^2 + (col_s - col_a)^2, an integer <= 2 * 127^2 = 32258; a frame without events
// has d2 = 2^31 - 1 (int32 output) / 0xFFFF (the uint16 maps of the workspace) everywhere.
//
// distance_frame_kernel: one workgroup per frame.  The frame is read from HBM ONCE: every pixel becomes one byte in LDS, bit k of which
// says "event of threshold k" (K <= 8).  Then, per threshold:
//   count   the events of the frame (integer workgroup sum).  A frame without events skips both passes: nothing is computed on it.
//   columns one thread per column scans it downwards and upwards: g = the distance to the nearest event of the same column, saturating at
//           256 ("none"; real distances are <= 127).  g^2 goes to LDS as uint16, 0xFFFF for a column without events: in the row pass
//           0xFFFF + 127^2 = 81664 stays far below 2^31, and, the frame having an event, some column offers a real candidate <= 32258.
//   rows    d2[y][x] = min over x' of g2[y][x'] + (x - x')^2, the direct minimum over the W candidates (int32).  The threads of a wave
//           hold consecutive x of one row and read the same g2[y][x']: a broadcast LDS read.
//   The result goes out as int32 (pd_distance_map), as uint16 to the workspace (the target's frames of an update), or is used in place
//   against the target's map of the workspace (the members' frames): per pixel sqrt of the two integers in fp64, the sums over the
//   event pixels, the integer maximum, Baddeley's squared differences.  Per-thread partials over a fixed pixel set, wave butterflies,
//   waves in order: the same pair gives the same bits.  No atomics of any kind.
// LDS (dynamic, sized from H and W): g2 2 H W + mask H W + 224 bytes of reduction cells: 49 376 bytes at 128 x 128.
//
// distance_fold_kernel: grid (T', K): the per-pair values of one step and one threshold -> the state, fp64, per-thread partials over a
// fixed pair set and a fixed tree (the construction of objects.hip's pair kernel).
//
// pd_distance_update is three launches in one stream: the target's N T frames (maps -> workspace), the members' M N T frames (pair values
// -> workspace), the fold.  The target's maps are made once for all members.
#include "axes.h"
#include "common.h"

namespace {

constexpr int DM_THREADS = 512, DM_WAVES = DM_THREADS / 64;
constexpr int DM_MAX = 128;                     // the largest side
constexpr int DM_MAXK = 8;                      // thresholds: one bit of the mask byte each
constexpr int DM_MAXM = 512;
constexpr int DM_NO_EVENT = 0x7fffffff;         // int32 d2 of a frame without events
constexpr int DM_FAR = 0xFFFF;                  // uint16: g^2 of a column without events, d2 of a frame without events
constexpr int DM_NONE = 256;                    // column scan: no event met yet
constexpr int DM_REC = 4;                       // doubles per (member frame, threshold): med_miss, med_false, hausdorff, baddeley

struct DmSource {
  const float* base;
  int64_t s_lead, s_n, s_t, s_h, s_w;           // element strides: leading (member) axis, N, T, H, W
};

struct DmParams {
  int h, w, k;
  int64_t n, t;                                 // frames per leading index: n * t
  float divisor;
  float thr[DM_MAXK];
  int use_cutoff;
  double cutoff;
  int64_t info_base, target_base;               // info rows of this launch's first frame / of the target's first frame
};

int64_t dm_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
__device__ __forceinline__ int dm_align16_dev(int v) { return (v + 15) & ~15; }

size_t dm_lds_bytes(int H, int W) {
  return (size_t)dm_align16(2 * (int64_t)H * W) + (size_t)dm_align16((int64_t)H * W) + sizeof(double) * 3 * DM_WAVES + sizeof(int) * DM_WAVES;
}

// sums over the workgroup in a fixed order, the same bits in every thread (called by every thread)
__device__ __forceinline__ void dm_block_sum3(double (&v)[3], double* __restrict__ red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int n = 0; n < 3; ++n) v[n] = wave_sum_f64(v[n]);
  __syncthreads();                                             // the last reader of red is done
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < 3; ++n) red[n * DM_WAVES + wave] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    double a = red[n * DM_WAVES];
#pragma unroll
    for (int w = 1; w < DM_WAVES; ++w) a += red[n * DM_WAVES + w];
    v[n] = a;
  }
}

template <bool MAX>
__device__ __forceinline__ int dm_block_int(int v, int* __restrict__ ired) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = MAX ? max(v, u) : v + u;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) ired[threadIdx.x >> 6] = v;
  __syncthreads();
  int a = ired[0];
#pragma unroll
  for (int w = 1; w < DM_WAVES; ++w) a = MAX ? max(a, ired[w]) : a + ired[w];
  return a;
}

// d2_out: NULL or int32 [frames][H W] (k = 1).  maps_out: NULL or uint16 [frames][K][H W].  tmaps: NULL or the target's maps, uint16
// [n t][K][H W]; then rec [frames][K][DM_REC] gets the pair values.  info: NULL or int32 rows of K + 1: events per threshold, non-finite flag.
__global__ void __launch_bounds__(DM_THREADS) distance_frame_kernel(DmSource src, DmParams q, int* __restrict__ d2_out,
                                                                    unsigned short* __restrict__ maps_out,
                                                                    const unsigned short* __restrict__ tmaps, int* info,
                                                                    double* __restrict__ rec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dm_lds[];
  const int tid = threadIdx.x;
  const int H = q.h, W = q.w, HW = H * W, K = q.k;
  unsigned short* g2 = (unsigned short*)dm_lds;
  unsigned char* mask = dm_lds + dm_align16_dev(2 * HW);
  double* red = (double*)(mask + dm_align16_dev(HW));
  int* ired = (int*)(red + 3 * DM_WAVES);

  const int64_t f = blockIdx.x, per = q.n * q.t;
  const float* __restrict__ frame = src.base + (f / per) * src.s_lead + ((f % per) / q.t) * src.s_n + (f % q.t) * src.s_t;

  // ---- the frame, once: one byte per pixel, bit k = event of threshold k
  int nonfinite = 0;
  for (int p = tid; p < HW; p += DM_THREADS) {
    const int y = p / W, x = p - y * W;
    const float v = frame[y * src.s_h + x * src.s_w];
    nonfinite |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    const float sv = v / q.divisor;                            // IEEE division, as pd_sevir_skill_counts
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < DM_MAXK; ++k)
      if (k < K && sv >= q.thr[k]) bits |= 1u << k;
    mask[p] = (unsigned char)bits;
  }
  nonfinite = __syncthreads_or(nonfinite);
  int* finfo = info ? info + (q.info_base + f) * (K + 1) : nullptr;
  const int* tinfo = tmaps ? info + (q.target_base + f % per) * (K + 1) : nullptr;
  if (finfo && tid == 0) finfo[K] = nonfinite;
  // an update skips the pairs of a frame with a non-finite pixel: no map is made of it, and none is read
  if (!d2_out && (nonfinite || (tinfo && tinfo[K] != 0))) return;

  for (int k = 0; k < K; ++k) {
    int cnt = 0;
    for (int p = tid; p < HW; p += DM_THREADS) cnt += (mask[p] >> k) & 1;
    cnt = dm_block_int<false>(cnt, ired);                      // its barriers also end the row pass of the threshold before
    if (finfo && tid == 0) finfo[k] = cnt;

    if (cnt > 0) {
      if (tid < W) {
        int d = DM_NONE;
        for (int y = 0; y < H; ++y) {
          d = ((mask[y * W + tid] >> k) & 1) ? 0 : min(d + 1, DM_NONE);
          g2[y * W + tid] = (unsigned short)d;
        }
        d = DM_NONE;
        for (int y = H - 1; y >= 0; --y) {
          d = ((mask[y * W + tid] >> k) & 1) ? 0 : min(d + 1, DM_NONE);
          const int m = min(d, (int)g2[y * W + tid]);
          g2[y * W + tid] = (unsigned short)(m >= DM_NONE ? DM_FAR : m * m);
        }
      }
      __syncthreads();
    }

    const int cnt_o = tinfo ? tinfo[k] : 0;
    const bool both = cnt > 0 && cnt_o > 0;
    const unsigned short* __restrict__ omap = tmaps ? tmaps + ((f % per) * K + k) * HW : nullptr;
    double a[3] = {0.0, 0.0, 0.0};                             // sum over O of d_F, sum over F of d_O, sum of (w(d_F) - w(d_O))^2
    int far = 0;
    for (int p = tid; p < HW; p += DM_THREADS) {
      int best = DM_FAR;
      if (cnt > 0) {
        const int y = p / W, x = p - y * W;
        const unsigned short* __restrict__ row = g2 + y * W;
        best = DM_NO_EVENT;
        for (int xx = 0; xx < W; ++xx) {
          const int dx = x - xx;
          best = min(best, (int)row[xx] + dx * dx);
        }
      }
      if (d2_out) d2_out[f * HW + p] = cnt > 0 ? best : DM_NO_EVENT;
      if (maps_out) maps_out[(f * K + k) * HW + p] = (unsigned short)best;
      if (omap && (both || q.use_cutoff)) {
        const int o = omap[p];
        const double df = cnt > 0 ? sqrt((double)best) : (double)INFINITY;
        const double dO = cnt_o > 0 ? sqrt((double)o) : (double)INFINITY;
        const double diff = q.use_cutoff ? fmin(df, q.cutoff) - fmin(dO, q.cutoff) : df - dO;
        a[2] += diff * diff;
        if (both) {
          if (o == 0) a[0] += df, far = max(far, best);
          if (best == 0) a[1] += dO, far = max(far, o);
        }
      }
    }
    if (omap) {
      dm_block_sum3(a, red);
      far = dm_block_int<true>(far, ired);
      if (tid == 0) {
        double* o = rec + (f * K + k) * DM_REC;
        o[0] = both ? a[0] / (double)cnt_o : 0.0;
        o[1] = both ? a[1] / (double)cnt : 0.0;
        o[2] = both ? sqrt((double)far) : 0.0;
        o[3] = (both || q.use_cutoff) ? sqrt(a[2] / ((double)H * (double)W)) : 0.0;
      }
    }
  }
}

// grid (T', K): block (tk, k) folds the (member, n[, t]) pairs of its step at its threshold.  info: M N T member rows, then N T target rows.
// sums [4][K][T']: med_miss, med_false, hausdorff, baddeley;  counts [6][K][T']: pairs, skipped, both non-empty, baddeley defined, event
// pixels in pred, in target.
__global__ void __launch_bounds__(256) distance_fold_kernel(const double* __restrict__ rec, const int* __restrict__ info, int M, int64_t N,
                                                            int64_t T, int K, int keep_seq, int use_cutoff, double* __restrict__ sums,
                                                            long long* __restrict__ counts) {
  __shared__ double rs[256];
  __shared__ long long rc[256];
  const int tid = threadIdx.x, tk = blockIdx.x, k = blockIdx.y;
  const int64_t Tk = keep_seq ? T : 1;
  const int64_t total = keep_seq ? (int64_t)M * N : (int64_t)M * N * T;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  long long c[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = tid; i < total; i += 256) {
    int64_t m, n, t;
    if (keep_seq) m = i / N, n = i % N, t = tk;
    else m = i / (N * T), n = (i / T) % N, t = i % T;
    const int64_t fm = (m * N + n) * T + t;
    const int* F = info + fm * (K + 1);
    const int* O = info + (((int64_t)M * N + n) * T + t) * (K + 1);
    if (F[K] != 0 || O[K] != 0) {
      c[1] += 1;
      continue;
    }
    const double* r = rec + (fm * K + k) * DM_REC;
    const bool both = F[k] > 0 && O[k] > 0;
    c[0] += 1;
    c[4] += F[k];
    c[5] += O[k];
    if (both) a[0] += r[0], a[1] += r[1], a[2] += r[2], c[2] += 1;
    if (both || use_cutoff) a[3] += r[3], c[3] += 1;
  }
  const int64_t cell = (int64_t)k * Tk + tk, plane = (int64_t)K * Tk;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rs[tid] = a[j];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) rs[tid] += rs[tid + h];
      __syncthreads();
    }
    if (tid == 0) sums[j * plane + cell] += rs[0];
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    rc[tid] = c[j];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) rc[tid] += rc[tid + h];
      __syncthreads();
    }
    if (tid == 0) counts[j * plane + cell] += rc[0];
    __syncthreads();
  }
}

// frames of a call with M leading members (M = 0: the frames of `sizes` alone); -1: unsupported
int64_t dm_frames(int M, const int64_t* sizes) {
  Axes5 g;
  if (M < 0 || M > DM_MAXM || !read_axes(sizes, g) || g.c != 1 || g.h > DM_MAX || g.w > DM_MAX) return -1;
  const double frames = (double)(M + 1) * (double)g.n * (double)g.t;
  return frames > (double)(1 << 30) ? -1 : (int64_t)(M + 1) * g.n * g.t;
}

// the workspace of an update: pair values, info rows, the target's maps
struct DmWs {
  int64_t rec, info, maps, bytes;               // byte offsets and the size
};

bool dm_ws(int M, int K, const int64_t* sizes, DmWs& w) {
  const int64_t frames = dm_frames(M, sizes);
  if (frames < 0 || M < 1 || K < 1 || K > DM_MAXK) return false;
  const int64_t ft = sizes[0] * sizes[1], fm = frames - ft, hw = sizes[2] * sizes[3];
  w.rec = 0;
  w.info = fm * K * DM_REC * (int64_t)sizeof(double);
  w.maps = dm_align16(w.info + frames * (K + 1) * (int64_t)sizeof(int));
  w.bytes = dm_align16(w.maps + ft * K * hw * (int64_t)sizeof(unsigned short));
  return true;
}

int dm_check(const char* who, const int64_t* sizes, float divisor) {
  for (int i = 0; i < 5; ++i) PD_CHECK_ARG(sizes[i] >= 1, "%s: axis %d has size %lld", who, i, (long long)sizes[i]);
  PD_CHECK_ARG(sizes[4] == 1, "%s: C = %lld; distance maps are made of one channel", who, (long long)sizes[4]);
  PD_CHECK_ARG(sizes[2] <= DM_MAX && sizes[3] <= DM_MAX,
               "%s: %lld x %lld frames: the maps of a frame live in LDS, sides up to %d are supported", who, (long long)sizes[2],
               (long long)sizes[3], DM_MAX);
  PD_CHECK_ARG(divisor > 0.0f && divisor <= 3.4e38f, "%s: divisor = %g (positive and finite)", who, (double)divisor);
  return PD_OK;
}

int dm_launch(DmSource src, int64_t frames, const DmParams& q, int* d2, unsigned short* maps_out, const unsigned short* tmaps, int* info,
              double* rec, hipStream_t stream) {
  const int lds = (int)dm_lds_bytes(q.h, q.w);
  static bool lds_set[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_distance", (const void*)distance_frame_kernel, (int)dm_lds_bytes(DM_MAX, DM_MAX), lds_set)) return rc;
  hipLaunchKernelGGL(distance_frame_kernel, dim3((unsigned)frames), dim3(DM_THREADS), lds, stream, src, q, d2, maps_out, tmaps, info, rec);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

}  // namespace

extern "C" int64_t pd_distance_ws_bytes(int M, int K, const int64_t* sizes) {
  DmWs w;
  return dm_ws(M, K, sizes, w) ? w.bytes : -1;
}

extern "C" int pd_distance_map(const float* frames, const int64_t* sizes, const int64_t* strides, float threshold, float divisor, int* d2,
                               pd_stream_t stream) {
  PD_CHECK_ARG(frames && sizes && strides && d2, "pd_distance_map: null pointer");
  if (int rc = dm_check("pd_distance_map", sizes, divisor)) return rc;
  const int64_t nf = dm_frames(0, sizes);
  PD_CHECK_ARG(nf > 0, "pd_distance_map: too many frames in one call");
  const int64_t span = axes_span(sizes, strides, 4, 1, 0);
  PD_CHECK_ARG(span > 0, "pd_distance_map: negative stride");
  PD_CHECK_ARG(!bytes_overlap(d2, nf * sizes[2] * sizes[3] * (int64_t)sizeof(int), frames, span), "pd_distance_map: d2 aliases the frames");
  DmParams q = {};
  q.h = (int)sizes[2], q.w = (int)sizes[3], q.k = 1, q.n = sizes[0], q.t = sizes[1];
  q.divisor = divisor, q.thr[0] = threshold;
  return dm_launch(DmSource{frames, 0, strides[0], strides[1], strides[2], strides[3]}, nf, q, d2, nullptr, nullptr, nullptr, nullptr,
                   (hipStream_t)stream);
}

extern "C" int pd_distance_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                                  const int64_t* target_strides, const float* thresholds, int K, float divisor, int use_cutoff,
                                  double cutoff, int keep_seq, double* sums, long long* counts, void* ws, int64_t ws_bytes,
                                  pd_stream_t stream) {
  PD_CHECK_ARG(pred && target && sizes && pred_strides && target_strides && thresholds && sums && counts && ws,
               "pd_distance_update: null pointer");
  PD_CHECK_ARG(M >= 1 && M <= DM_MAXM, "pd_distance_update: %d members (supported: 1 .. %d)", M, DM_MAXM);
  PD_CHECK_ARG(K >= 1 && K <= DM_MAXK, "pd_distance_update: %d thresholds (supported: 1 .. %d)", K, DM_MAXK);
  if (int rc = dm_check("pd_distance_update", sizes, divisor)) return rc;
  PD_CHECK_ARG(!use_cutoff || (cutoff > 0.0 && cutoff <= 1.7e308), "pd_distance_update: cutoff = %g (positive and finite)", cutoff);
  DmWs w;
  PD_CHECK_ARG(dm_ws(M, K, sizes, w), "pd_distance_update: too many frames in one update");
  PD_CHECK_ARG(ws_bytes >= w.bytes, "pd_distance_update: workspace of %lld bytes < %lld", (long long)ws_bytes, (long long)w.bytes);
  PD_CHECK_ARG(((uintptr_t)ws & 15) == 0, "pd_distance_update: the workspace is not 16-byte aligned");
  const int64_t pspan = axes_span(sizes, pred_strides + 1, 4, M, pred_strides[0]), tspan = axes_span(sizes, target_strides, 4, 1, 0);
  PD_CHECK_ARG(pspan > 0 && tspan > 0, "pd_distance_update: negative stride");
  const int64_t N = sizes[0], T = sizes[1], Tk = keep_seq ? T : 1;
  const int64_t sbytes = 4 * K * Tk * (int64_t)sizeof(double), cbytes = 6 * K * Tk * (int64_t)sizeof(long long);
  PD_CHECK_ARG(!bytes_overlap(ws, w.bytes, pred, pspan) && !bytes_overlap(ws, w.bytes, target, tspan) && !bytes_overlap(ws, w.bytes, sums, sbytes) &&
                   !bytes_overlap(ws, w.bytes, counts, cbytes),
               "pd_distance_update: the workspace aliases an input or the state");
  PD_CHECK_ARG(!bytes_overlap(sums, sbytes, pred, pspan) && !bytes_overlap(sums, sbytes, target, tspan) && !bytes_overlap(counts, cbytes, pred, pspan) &&
                   !bytes_overlap(counts, cbytes, target, tspan) && !bytes_overlap(sums, sbytes, counts, cbytes),
               "pd_distance_update: the state aliases an input");
  double* rec = (double*)((char*)ws + w.rec);
  int* info = (int*)((char*)ws + w.info);
  unsigned short* maps = (unsigned short*)((char*)ws + w.maps);
  DmParams q = {};
  q.h = (int)sizes[2], q.w = (int)sizes[3], q.k = K, q.n = N, q.t = T;
  q.divisor = divisor, q.use_cutoff = use_cutoff ? 1 : 0, q.cutoff = use_cutoff ? cutoff : 0.0;
  for (int k = 0; k < K; ++k) q.thr[k] = thresholds[k];
  const int64_t fm = (int64_t)M * N * T;
  q.info_base = fm, q.target_base = fm;
  if (int rc = dm_launch(DmSource{target, 0, target_strides[0], target_strides[1], target_strides[2], target_strides[3]}, N * T, q, nullptr,
                         maps, nullptr, info, nullptr, (hipStream_t)stream))
    return rc;
  q.info_base = 0;
  if (int rc = dm_launch(DmSource{pred, pred_strides[0], pred_strides[1], pred_strides[2], pred_strides[3], pred_strides[4]}, fm, q, nullptr,
                         nullptr, maps, info, rec, (hipStream_t)stream))
    return rc;
  hipLaunchKernelGGL(distance_fold_kernel, dim3((unsigned)Tk, (unsigned)K), dim3(256), 0, (hipStream_t)stream, (const double*)rec,
                     (const int*)info, M, N, T, K, keep_seq, q.use_cutoff, sums, counts);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
