// Intensity-scale verification: the Haar energies of the event fields of forecast / observation pairs and of their difference, per
// threshold and scale (Casati, Ross and Stephenson 2004; Casati 2010 for frames that are not dyadic).  Not in the reference.
//
// A frame is one (n, t) image of H x W pixels (C = 1, 1 <= H, W <= 128), addressed in place through the element strides of its axes.
// Event of threshold k: v[s] / divisor >= thr_k -- the IEEE division and comparison of pd_sevir_skill_counts; a NaN is never an event.
// The 0 / 1 event field sits at the top-left corner of an S x S field of zeros, S = 2^n the smallest power of two >= max(H, W, 2).
// Q_l(A), l = 0 .. n: the sum over the 2^l x 2^l blocks of (block sum of A)^2.  With I_F, I_O the event fields of a pair and Z = I_F - I_O,
// every block sum of Z is the block sum of I_F minus that of I_O, so Q(I_F), Q(I_O), Q(Z) come from the same two block sums.  All of it is
// integer arithmetic: a block sum is <= 4^l, a Q_l <= 4^(n + l) <= 2^28 (int32), the state int64.  The component energies of the score
// are differences of these integers, formed on the host (prediff_amd/scale_score.py).
//
// scale_frame_kernel: one workgroup of 8 waves per frame.  The frame is read from HBM ONCE for all K thresholds: a wave takes 64
// consecutive pixels of a row, and __ballot of the event test of threshold k is one 64-bit word of bit plane k in LDS (bits past W are
// zero, rows past H do not exist: the padding).  A plane is H x ceil(W / 64) words.  Then
//   target frames   the planes go to the workspace as they are;
//   member frames   the target's planes of the same (n, t) come from the workspace into LDS, and the (threshold, level) combinations
//                   are dealt to the waves.  Level 0: popcounts of f, o, f ^ o over the words.  Level l = 1 .. min(n, 6): a lane owns a
//                   block, its sum is __popcll of the block's 2^l bits of the word, added over the block's rows.  Level 7 (S = 128) is one
//                   block, the frame: the squares of the level-0 counts.  A wave butterfly adds the lanes' squares: no barrier, no atomics.
//   pd_scale_energy the same with one threshold and no target.
// LDS (static): the planes of F and of O, 2 x 8 thresholds x 128 rows x 2 words x 8 bytes = 32 768 bytes, and 256 bytes of the workgroup
// OR of the non-finite flag: 33 024 bytes (16 640 without a target).
//
// scale_fold_kernel: grid (T', K, 3): the per-pair records of one step, one threshold and one of F, O, Z -> the int64 state; per-thread
// partials over a fixed pair set, wave butterflies, waves in order.
//
// pd_scale_update is three launches in one stream: the target's N T frames (planes -> workspace), the members' M N T frames (records ->
// workspace), the fold.  The target's planes are made once for all members.
#include "axes.h"
#include "common.h"

namespace {

constexpr int SC_THREADS = 512, SC_WAVES = SC_THREADS / 64;
constexpr int SC_MAX = 128;                     // the largest side
constexpr int SC_MAXK = 8;                      // thresholds
constexpr int SC_MAXM = 512;
constexpr int SC_LEVELS = 8;                    // l = 0 .. 7
constexpr int SC_PLANE = SC_MAX * (SC_MAX / 64);             // words of one bit plane at 128 x 128
constexpr int SC_REC = 3 * SC_LEVELS;           // int32 per (member frame, threshold): Q(I_F), Q(I_O), Q(Z)

struct ScSource {
  const float* base;
  int64_t s_lead, s_n, s_t, s_h, s_w;           // element strides: leading (member) axis, N, T, H, W
};

struct ScParams {
  int h, w, k, levels;                          // levels: n, S = 2^n
  int64_t n, t;                                 // frames per leading index: n * t
  float divisor;
  float thr[SC_MAXK];
  int64_t info_base, target_base;               // info entries of this launch's first frame / of the target's first frame
};

int64_t sc_align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// n with 2^n the smallest power of two >= max(H, W, 2)
int sc_levels(int64_t H, int64_t W) {
  int n = 1;
  while (((int64_t)1 << n) < H || ((int64_t)1 << n) < W) ++n;
  return n;
}

__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// PAIR: member frames against the target's planes (tplanes) -> rec int32 [frames][K][3][8].  Else planes_out != NULL: the target's frames
// -> planes uint64 [frames][K][H words]; planes_out == NULL: q_out int64 [frames][8] of threshold 0.  info: NULL or one int32 per frame,
// the non-finite flag.
template <bool PAIR>
__global__ void __launch_bounds__(SC_THREADS) scale_frame_kernel(ScSource src, ScParams q, unsigned long long* __restrict__ planes_out,
                                                                 const unsigned long long* __restrict__ tplanes, int* info,
                                                                 int* __restrict__ rec, long long* __restrict__ q_out) {
  __shared__ unsigned long long fpl[SC_MAXK * SC_PLANE];
  __shared__ unsigned long long opl[PAIR ? SC_MAXK * SC_PLANE : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = q.h, W = q.w, K = q.k, n = q.levels;
  const int two = W > 64, NW = two + 1, words = H * NW;          // words of a row, of a plane

  const int64_t f = blockIdx.x, per = q.n * q.t;
  const float* __restrict__ frame = src.base + (f / per) * src.s_lead + ((f % per) / q.t) * src.s_n + (f % q.t) * src.s_t;

  // ---- the frame, once: word s of plane k = the events of threshold k among pixels 64 j .. 64 j + 63 of row y
  int nonfinite = 0;
  for (int s = wave; s < words; s += SC_WAVES) {
    const int y = s >> two, x = ((s & two) << 6) + lane;
    const bool in = x < W;
    const float v = in ? frame[y * src.s_h + x * src.s_w] : 0.0f;
    nonfinite |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    const float sv = v / q.divisor;                              // IEEE division, as pd_sevir_skill_counts
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < SC_MAXK; ++k)
      if (k < K) {
        const unsigned long long b = __ballot(in && sv >= q.thr[k]);
        if (lane == k) mine = b;
      }
    if (lane < K) fpl[lane * words + s] = mine;
  }
  nonfinite = __syncthreads_or(nonfinite);                       // and the planes are complete
  if (info && tid == 0) info[q.info_base + f] = nonfinite;

  if (!PAIR && planes_out) {
    for (int i = tid; i < K * words; i += SC_THREADS) planes_out[f * K * words + i] = fpl[i];
    return;
  }
  if (PAIR) {
    // an update skips the pairs of a frame with a non-finite pixel: no record is made of them, and none is read
    if (nonfinite || info[q.target_base + f % per] != 0) return;
    for (int i = tid; i < K * words; i += SC_THREADS) opl[i] = tplanes[(f % per) * K * words + i];
    __syncthreads();
  } else if (tid > n && tid < SC_LEVELS) {
    q_out[f * SC_LEVELS + tid] = 0;
  }

  // ---- (threshold, level) combinations, dealt to the waves; levels 0 .. min(n, 6), level 7 with level 0
  const int nl = min(n, 6) + 1;
  for (int c = wave; c < K * nl; c += SC_WAVES) {
    const int k = c / nl, l = c - k * nl;
    const unsigned long long* __restrict__ F = fpl + k * words;
    const unsigned long long* __restrict__ O = opl + (PAIR ? k * words : 0);
    int aF = 0, aO = 0, aZ = 0;
    if (l == 0) {
      for (int i = lane; i < words; i += 64) {
        const unsigned long long fw = F[i], ow = PAIR ? O[i] : 0ull;
        aF += __popcll(fw), aO += __popcll(ow), aZ += __popcll(fw ^ ow);
      }
    } else {
      const int b = 1 << l, nbx = (W + b - 1) >> l, nby = (H + b - 1) >> l;
      const unsigned long long bits = l == 6 ? ~0ull : (1ull << b) - 1;
      for (int it = lane; it < nby * nbx; it += 64) {
        const int by = it / nbx, x0 = (it - by * nbx) << l;
        const int word = x0 >> 6, sh = x0 & 63, y1 = min((by + 1) << l, H);
        int sF = 0, sO = 0;
        for (int y = by << l; y < y1; ++y) {
          sF += __popcll((F[y * NW + word] >> sh) & bits);
          if (PAIR) sO += __popcll((O[y * NW + word] >> sh) & bits);
        }
        aF += sF * sF, aO += sO * sO, aZ += (sF - sO) * (sF - sO);
      }
    }
    aF = sc_wave_sum(aF), aO = sc_wave_sum(aO), aZ = sc_wave_sum(aZ);
    if (lane == 0) {
      if (PAIR) {
        int* r = rec + (f * K + k) * SC_REC;
        r[l] = aF, r[SC_LEVELS + l] = aO, r[2 * SC_LEVELS + l] = aZ;
        if (l == 0 && n == 7) r[7] = aF * aF, r[SC_LEVELS + 7] = aO * aO, r[2 * SC_LEVELS + 7] = (aF - aO) * (aF - aO);
      } else {
        q_out[f * SC_LEVELS + l] = aF;
        if (l == 0 && n == 7) q_out[f * SC_LEVELS + 7] = (long long)aF * aF;
      }
    }
  }
}

// grid (T', K, 3): block (tk, k, a) folds Q_l of field a (F, O, Z) of the (member, n[, t]) pairs of its step at its threshold.
// info: M N T member entries, then N T target entries.  energy [3][K][8][T'];  counts [2][T']: pairs, skipped (block k = 0, a = 0).
__global__ void __launch_bounds__(256) scale_fold_kernel(const int* __restrict__ rec, const int* __restrict__ info, int M, int64_t N, int64_t T,
                                                         int K, int n, int keep_seq, long long* __restrict__ energy,
                                                         long long* __restrict__ counts) {
  __shared__ long long red[4][SC_LEVELS + 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tk = blockIdx.x, k = blockIdx.y, a = blockIdx.z;
  const int64_t Tk = keep_seq ? T : 1;
  const int64_t total = keep_seq ? (int64_t)M * N : (int64_t)M * N * T;
  long long v[SC_LEVELS + 2] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // Q_0 .. Q_7, pairs, skipped
  for (int64_t i = tid; i < total; i += 256) {
    int64_t m, nn, t;
    if (keep_seq) m = i / N, nn = i % N, t = tk;
    else m = i / (N * T), nn = (i / T) % N, t = i % T;
    const int64_t fm = (m * N + nn) * T + t;
    if (info[fm] != 0 || info[((int64_t)M * N + nn) * T + t] != 0) {
      v[SC_LEVELS + 1] += 1;
      continue;
    }
    v[SC_LEVELS] += 1;
    const int* r = rec + (fm * K + k) * SC_REC + a * SC_LEVELS;
#pragma unroll
    for (int l = 0; l < SC_LEVELS; ++l)
      if (l <= n) v[l] += r[l];
  }
#pragma unroll
  for (int j = 0; j < SC_LEVELS + 2; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o, 64);
    if (lane == 0) red[wave][j] = v[j];
  }
  __syncthreads();
  if (tid < SC_LEVELS + 2) {
    const long long s = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (tid <= n && tid < SC_LEVELS) energy[(((int64_t)a * K + k) * SC_LEVELS + tid) * Tk + tk] += s;
    if (tid >= SC_LEVELS && k == 0 && a == 0) counts[(tid - SC_LEVELS) * Tk + tk] += s;
  }
}

// frames of a call with M leading members (M = 0: the frames of `sizes` alone); -1: unsupported
int64_t sc_frames(int M, const int64_t* sizes) {
  Axes5 g;
  if (M < 0 || M > SC_MAXM || !read_axes(sizes, g) || g.c != 1 || g.h > SC_MAX || g.w > SC_MAX) return -1;
  const double frames = (double)(M + 1) * (double)g.n * (double)g.t;
  return frames > (double)(1 << 30) ? -1 : (int64_t)(M + 1) * g.n * g.t;
}

// the workspace of an update: records, non-finite flags, the target's planes
struct ScWs {
  int64_t rec, info, planes, bytes;             // byte offsets and the size
};

bool sc_ws(int M, int K, const int64_t* sizes, ScWs& w) {
  const int64_t frames = sc_frames(M, sizes);
  if (frames < 0 || M < 1 || K < 1 || K > SC_MAXK) return false;
  const int64_t ft = sizes[0] * sizes[1], fm = frames - ft, words = sizes[2] * ((sizes[3] + 63) / 64);
  w.rec = 0;
  w.info = fm * K * SC_REC * (int64_t)sizeof(int);
  w.planes = sc_align16(w.info + frames * (int64_t)sizeof(int));
  w.bytes = sc_align16(w.planes + ft * K * words * (int64_t)sizeof(unsigned long long));
  return true;
}

int sc_check(const char* who, const int64_t* sizes, float divisor) {
  for (int i = 0; i < 5; ++i) PD_CHECK_ARG(sizes[i] >= 1, "%s: axis %d has size %lld", who, i, (long long)sizes[i]);
  PD_CHECK_ARG(sizes[4] == 1, "%s: C = %lld; event fields are made of one channel", who, (long long)sizes[4]);
  PD_CHECK_ARG(sizes[2] <= SC_MAX && sizes[3] <= SC_MAX,
               "%s: %lld x %lld frames: the bit planes of a frame live in LDS, sides up to %d are supported", who, (long long)sizes[2],
               (long long)sizes[3], SC_MAX);
  PD_CHECK_ARG(divisor > 0.0f && divisor <= 3.4e38f, "%s: divisor = %g (positive and finite)", who, (double)divisor);
  return PD_OK;
}

ScParams sc_params(const int64_t* sizes, int K, float divisor) {
  ScParams q = {};
  q.h = (int)sizes[2], q.w = (int)sizes[3], q.k = K, q.levels = sc_levels(sizes[2], sizes[3]);
  q.n = sizes[0], q.t = sizes[1], q.divisor = divisor;
  return q;
}

}  // namespace

extern "C" int64_t pd_scale_ws_bytes(int M, int K, const int64_t* sizes) {
  ScWs w;
  return sc_ws(M, K, sizes, w) ? w.bytes : -1;
}

extern "C" int pd_scale_energy(const float* frames, const int64_t* sizes, const int64_t* strides, float threshold, float divisor,
                               long long* q_out, pd_stream_t stream) {
  PD_CHECK_ARG(frames && sizes && strides && q_out, "pd_scale_energy: null pointer");
  if (int rc = sc_check("pd_scale_energy", sizes, divisor)) return rc;
  const int64_t nf = sc_frames(0, sizes);
  PD_CHECK_ARG(nf > 0, "pd_scale_energy: too many frames in one call");
  const int64_t span = axes_span(sizes, strides, 4, 1, 0);
  PD_CHECK_ARG(span > 0, "pd_scale_energy: negative stride");
  PD_CHECK_ARG(!bytes_overlap(q_out, nf * SC_LEVELS * (int64_t)sizeof(long long), frames, span), "pd_scale_energy: q_out aliases the frames");
  ScParams q = sc_params(sizes, 1, divisor);
  q.thr[0] = threshold;
  hipLaunchKernelGGL(scale_frame_kernel<false>, dim3((unsigned)nf), dim3(SC_THREADS), 0, (hipStream_t)stream,
                     ScSource{frames, 0, strides[0], strides[1], strides[2], strides[3]}, q, (unsigned long long*)nullptr,
                     (const unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr, q_out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_scale_update(const float* pred, const float* target, int M, const int64_t* sizes, const int64_t* pred_strides,
                               const int64_t* target_strides, const float* thresholds, int K, float divisor, int keep_seq,
                               long long* energy, long long* counts, void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(pred && target && sizes && pred_strides && target_strides && thresholds && energy && counts && ws,
               "pd_scale_update: null pointer");
  PD_CHECK_ARG(M >= 1 && M <= SC_MAXM, "pd_scale_update: %d members (supported: 1 .. %d)", M, SC_MAXM);
  PD_CHECK_ARG(K >= 1 && K <= SC_MAXK, "pd_scale_update: %d thresholds (supported: 1 .. %d)", K, SC_MAXK);
  if (int rc = sc_check("pd_scale_update", sizes, divisor)) return rc;
  ScWs w;
  PD_CHECK_ARG(sc_ws(M, K, sizes, w), "pd_scale_update: too many frames in one update");
  PD_CHECK_ARG(ws_bytes >= w.bytes, "pd_scale_update: workspace of %lld bytes < %lld", (long long)ws_bytes, (long long)w.bytes);
  PD_CHECK_ARG(((uintptr_t)ws & 15) == 0, "pd_scale_update: the workspace is not 16-byte aligned");
  const int64_t pspan = axes_span(sizes, pred_strides + 1, 4, M, pred_strides[0]), tspan = axes_span(sizes, target_strides, 4, 1, 0);
  PD_CHECK_ARG(pspan > 0 && tspan > 0, "pd_scale_update: negative stride");
  const int64_t N = sizes[0], T = sizes[1], Tk = keep_seq ? T : 1;
  const int64_t ebytes = 3 * K * SC_LEVELS * Tk * (int64_t)sizeof(long long), cbytes = 2 * Tk * (int64_t)sizeof(long long);
  PD_CHECK_ARG(!bytes_overlap(ws, w.bytes, pred, pspan) && !bytes_overlap(ws, w.bytes, target, tspan) &&
                   !bytes_overlap(ws, w.bytes, energy, ebytes) && !bytes_overlap(ws, w.bytes, counts, cbytes),
               "pd_scale_update: the workspace aliases an input or the state");
  PD_CHECK_ARG(!bytes_overlap(energy, ebytes, pred, pspan) && !bytes_overlap(energy, ebytes, target, tspan) &&
                   !bytes_overlap(counts, cbytes, pred, pspan) && !bytes_overlap(counts, cbytes, target, tspan) &&
                   !bytes_overlap(energy, ebytes, counts, cbytes),
               "pd_scale_update: the state aliases an input");
  int* rec = (int*)((char*)ws + w.rec);
  int* info = (int*)((char*)ws + w.info);
  unsigned long long* planes = (unsigned long long*)((char*)ws + w.planes);
  ScParams q = sc_params(sizes, K, divisor);
  for (int k = 0; k < K; ++k) q.thr[k] = thresholds[k];
  const int64_t fm = (int64_t)M * N * T;
  q.info_base = fm, q.target_base = fm;
  hipLaunchKernelGGL(scale_frame_kernel<false>, dim3((unsigned)(N * T)), dim3(SC_THREADS), 0, (hipStream_t)stream,
                     ScSource{target, 0, target_strides[0], target_strides[1], target_strides[2], target_strides[3]}, q, planes,
                     (const unsigned long long*)nullptr, info, (int*)nullptr, (long long*)nullptr);
  PD_CHECK_LAUNCH();
  q.info_base = 0;
  hipLaunchKernelGGL(scale_frame_kernel<true>, dim3((unsigned)fm), dim3(SC_THREADS), 0, (hipStream_t)stream,
                     ScSource{pred, pred_strides[0], pred_strides[1], pred_strides[2], pred_strides[3], pred_strides[4]}, q,
                     (unsigned long long*)nullptr, (const unsigned long long*)planes, info, rec, (long long*)nullptr);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(scale_fold_kernel, dim3((unsigned)Tk, (unsigned)K, 3), dim3(256), 0, (hipStream_t)stream, (const int*)rec,
                     (const int*)info, M, N, T, K, q.levels, keep_seq, energy, counts);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
