// Probability matching: the stable rank order of every frame (pd_rank_frames), CDF matching of forecast frames onto a reference frame
// (pd_cdf_match; pysteps' nonparam_match_empirical_cdf with its wet-area adjustment) and the probability-matched mean of an ensemble
// (pd_pmm; Ebert 2001, Mon. Wea. Rev. 129, 2461).  Not in the reference.  The definitions are the module docstring of
// prediff_amd/probability_matching.py; every result is a selection of input values, so everything here is exact.
//
// A frame is n = H W <= 16384 contiguous fp32 pixels.  ORDER is one thing everywhere: ascending by the exact fp32 value, ties by ascending
// pixel index.  Values are compared as 32-bit integer keys (pm_key: sign-magnitude -> offset binary, -0.0 folded onto +0.0), never as
// floats, so denormals order by their exact value whatever the denormal mode of the float compares.  A key with its pixel index in the
// low half of a 64-bit word is unique per frame: ANY correct sort of those words is the stable order, so the network need not be stable.
//
// pm_sort_lds<K>: bitonic sort of npad = 2^a >= 64 words in LDS (the frame padded with a sentinel above every finite key), one workgroup
// of 1024 threads.  A stage (k, j) compares word i with word i ^ j.  The strides j <= 32 stay inside 64 consecutive words = one wave:
// they run in registers with wave shuffles, no LDS traffic (all 21 stages of k <= 64 in one sweep, and the last six of every later k).
// The strides j >= 64 go through LDS two at a time (four words per thread: strides j and j / 2 in one read-modify-write) or one at a
// time when a single one is left.  All LDS accesses are 4 / 8 bytes per lane at consecutive addresses: conflict-free.  At 16384 64-bit
// words that is 20 + 9 sweeps over 128 KiB instead of 105.
//
// pm_rank_kernel     one workgroup per frame: 64-bit sort -> order, sorted (the ORIGINAL bits, gathered from the frame: -0.0 stays).
// pm_sort_keys_kernel  one workgroup per frame: 32-bit keys-only sort into the workspace (the reference frames of pd_cdf_match, each
//                    sorted ONCE however many forecast frames share it; the member frames of pd_pmm), and the frame's non-finite flag.
// pm_match_kernel    one workgroup per forecast frame: 64-bit sort, n_x by a binary search of the threshold in the sorted words, then
//                    out[order[r]] = the reference's r-th key, capped at the threshold below rank n - n_x.
// pm_merge_kernel    pd_pmm: one pass of a merge sort over the M sorted member frames of every (b, t), run length L -> 2 L, by merge
//                    path: every thread finds its diagonal by binary search and merges PM_VT outputs.  ceil(log2 M) passes ping-pong
//                    between the two halves of the workspace and leave P, the pooled M n keys in ascending order: exact order
//                    statistics, no histogram.
// pm_pmm_kernel      one workgroup per (b, t): the member mean (fp64 sum in member order, fp64 division, one rounding), its 64-bit
//                    sort, out[order_mean[r]] = P[r M + M / 2].
// No atomics anywhere, no inter-workgroup communication inside a launch: the same inputs give the same bits, a frame alone gives the bits
// it gives in a batch.  A frame with a non-finite pixel is never ordered (its words are sorted like any others and then not used).
#include "common.h"

namespace {

constexpr int PM_THREADS = 1024, PM_WAVES = PM_THREADS / 64;
constexpr int PM_MAX_N = 16384;                 // pixels per frame: 16384 64-bit words = 128 KiB of LDS
constexpr int PM_MAX_M = 512;
constexpr int PM_LDS_LIMIT = PM_MAX_N * 8;
constexpr int PM_ILP = 4;                       // 64-word chunks a wave holds in registers at once
constexpr int PM_VT = 8;                        // outputs per thread of a merge pass
constexpr int PM_MERGE_THREADS = 256;
constexpr int64_t PM_MAX_TOTAL = (int64_t)1 << 31;   // frames * M * n of one call

// fp32 bits -> a key whose unsigned order is the order of the values; -0.0 and +0.0 share a key
__device__ __forceinline__ uint32_t pm_key(uint32_t u) {
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// key -> fp32 bits (+0.0 for the shared zero key)
__device__ __forceinline__ uint32_t pm_unkey(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
__device__ __forceinline__ bool pm_nonfinite(uint32_t u) { return (u & 0x7f800000u) == 0x7f800000u; }
// host twin of pm_key (the threshold)
uint32_t pm_key_host(float f) {
  union { float f; uint32_t u; } c;
  c.f = f;
  uint32_t u = c.u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename K> __device__ __forceinline__ K pm_shfl_xor(K v, int j);
template <> __device__ __forceinline__ uint32_t pm_shfl_xor<uint32_t>(uint32_t v, int j) { return (uint32_t)__shfl_xor((int)v, j, 64); }
template <> __device__ __forceinline__ uint64_t pm_shfl_xor<uint64_t>(uint64_t v, int j) {
  return (uint64_t)__shfl_xor((unsigned long long)v, j, 64);
}

// one compare-exchange stage of stride j <= 32 inside a wave: lane holds word i, `up`: its block sorts ascending
template <typename K> __device__ __forceinline__ K pm_cx_lane(K v, int j, bool up, int lane) {
  const K p = pm_shfl_xor<K>(v, j);
  const bool lower = (lane & j) == 0;
  const K lo = v < p ? v : p, hi = v < p ? p : v;
  return lower == up ? lo : hi;
}
template <typename K> __device__ __forceinline__ void pm_cx(K& a, K& b, bool up) {
  const K lo = a < b ? a : b, hi = a < b ? b : a;
  a = up ? lo : hi;
  b = up ? hi : lo;
}

// The register stages of every 64-word chunk: FIRST: all 21 stages of k = 2 .. 64; else the strides 32 .. 1 of stage k.  A wave works on
// PM_ILP chunks at once: the shuffles of one chunk are a dependent chain, those of different chunks are not.
template <typename K, bool FIRST> __device__ __forceinline__ void pm_wave_stages(K* s, int chunks, int k) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c < chunks; c += PM_ILP * PM_WAVES) {
    K v[PM_ILP];
    int i[PM_ILP];
#pragma unroll
    for (int u = 0; u < PM_ILP; ++u) {
      i[u] = ((c + u * PM_WAVES) << 6) | lane;
      v[u] = c + u * PM_WAVES < chunks ? s[i[u]] : (K)0;
    }
    if (FIRST) {
#pragma unroll
      for (int kk = 2; kk <= 64; kk <<= 1)
#pragma unroll
        for (int j = kk >> 1; j > 0; j >>= 1)
#pragma unroll
          for (int u = 0; u < PM_ILP; ++u) v[u] = pm_cx_lane<K>(v[u], j, (i[u] & kk) == 0, lane);
    } else {
#pragma unroll
      for (int j = 32; j > 0; j >>= 1)
#pragma unroll
        for (int u = 0; u < PM_ILP; ++u) v[u] = pm_cx_lane<K>(v[u], j, (i[u] & k) == 0, lane);
    }
#pragma unroll
    for (int u = 0; u < PM_ILP; ++u)
      if (c + u * PM_WAVES < chunks) s[i[u]] = v[u];
  }
}

// ascending sort of s[0 .. npad), npad a power of two >= 64; called by all PM_THREADS threads; s is complete and visible on return
template <typename K> __device__ void pm_sort_lds(K* s, int npad) {
  const int tid = threadIdx.x;
  const int chunks = npad >> 6;
  __syncthreads();
  pm_wave_stages<K, true>(s, chunks, 0);                // k = 2 .. 64: 21 stages in registers
  for (int k = 128; k <= npad; k <<= 1) {
    int j = k >> 1;
    __syncthreads();
    while (j >= 64) {
      if (j >= 128) {                                   // strides j and j / 2 in one sweep
        const int h = j >> 1, lh = __ffs(h) - 1;
        for (int q = tid; q < (npad >> 2); q += PM_THREADS) {
          const int i0 = ((q >> lh) << (lh + 2)) | (q & (h - 1));
          const bool up = (i0 & k) == 0;
          K a0 = s[i0], a1 = s[i0 + h], a2 = s[i0 + j], a3 = s[i0 + j + h];
          pm_cx(a0, a2, up);
          pm_cx(a1, a3, up);
          pm_cx(a0, a1, up);
          pm_cx(a2, a3, up);
          s[i0] = a0, s[i0 + h] = a1, s[i0 + j] = a2, s[i0 + j + h] = a3;
        }
        j >>= 2;
      } else {                                          // j == 64 alone
        for (int q = tid; q < (npad >> 1); q += PM_THREADS) {
          const int i0 = ((q >> 6) << 7) | (q & 63);
          const bool up = (i0 & k) == 0;
          K a0 = s[i0], a1 = s[i0 + 64];
          pm_cx(a0, a1, up);
          s[i0] = a0, s[i0 + 64] = a1;
        }
        j >>= 1;
      }
      __syncthreads();
    }
    pm_wave_stages<K, false>(s, chunks, k);             // strides 32 .. 1 in registers
  }
  __syncthreads();
}

// the frame's (key, pixel) words into LDS, padded with the sentinel; returns whether the frame holds a non-finite pixel (all threads)
__device__ __forceinline__ int pm_load_words(const float* __restrict__ x, int n, int npad, uint64_t* s) {
  int bad = 0;
  for (int i = threadIdx.x; i < npad; i += PM_THREADS) {
    uint64_t w = ~0ull;
    if (i < n) {
      const uint32_t u = __float_as_uint(x[i]);
      bad |= pm_nonfinite(u);
      w = ((uint64_t)pm_key(u) << 32) | (uint32_t)i;
    }
    s[i] = w;
  }
  return __syncthreads_or(bad);
}

// grid: frames.  dynamic LDS: npad 64-bit words.
__global__ void __launch_bounds__(PM_THREADS) pm_rank_kernel(const float* __restrict__ x, int n, int npad, float* __restrict__ sorted,
                                                             int* __restrict__ order) {
  extern __shared__ uint64_t pm_smem64[];
  uint64_t* s = pm_smem64;
  const int64_t f = blockIdx.x;
  const float* __restrict__ xf = x + f * n;
  float* __restrict__ so = sorted + f * n;
  int* __restrict__ oo = order + f * n;
  if (pm_load_words(xf, n, npad, s)) {
    for (int r = threadIdx.x; r < n; r += PM_THREADS) so[r] = __uint_as_float(0x7fc00000u), oo[r] = -1;
    return;
  }
  pm_sort_lds<uint64_t>(s, npad);
  for (int r = threadIdx.x; r < n; r += PM_THREADS) {
    const int p = (int)(uint32_t)s[r];
    oo[r] = p;
    so[r] = xf[p];
  }
}

// grid: lead * per frames; frame f = (m, g) of src (m-major) goes to keys[(g * lead + m) * n ..): the members of one g end up side by side.
// flags: NULL, or one int per frame (non-finite pixel).  dynamic LDS: npad 32-bit words.
__global__ void __launch_bounds__(PM_THREADS) pm_sort_keys_kernel(const float* __restrict__ src, int64_t lead, int64_t per, int n, int npad,
                                                                  uint32_t* __restrict__ keys, int* __restrict__ flags) {
  extern __shared__ uint64_t pm_smem64[];
  uint32_t* s = (uint32_t*)pm_smem64;
  const int64_t f = blockIdx.x, m = f / per, g = f % per;
  const float* __restrict__ xf = src + f * n;
  int bad = 0;
  for (int i = threadIdx.x; i < npad; i += PM_THREADS) {
    uint32_t w = ~0u;
    if (i < n) {
      const uint32_t u = __float_as_uint(xf[i]);
      bad |= pm_nonfinite(u);
      w = pm_key(u);
    }
    s[i] = w;
  }
  bad = __syncthreads_or(bad);
  if (flags && threadIdx.x == 0) flags[f] = bad;
  pm_sort_lds<uint32_t>(s, npad);
  uint32_t* __restrict__ dst = keys + (g * lead + m) * n;
  for (int r = threadIdx.x; r < n; r += PM_THREADS) dst[r] = s[r];
}

// grid: lead * B * T forecast frames (m, b, t); its reference frame is (b, ref_T == 1 ? 0 : t).  dynamic LDS: npad 64-bit words.
__global__ void __launch_bounds__(PM_THREADS) pm_match_kernel(const float* __restrict__ x, const uint32_t* __restrict__ ref_keys,
                                                              const int* __restrict__ ref_flags, int64_t B, int T, int ref_T, int n, int npad,
                                                              uint32_t thr_key, float thr, int use_thr, float* __restrict__ out) {
  extern __shared__ uint64_t pm_smem64[];
  uint64_t* s = pm_smem64;
  const int64_t f = blockIdx.x;
  const int t = (int)(f % T);
  const int64_t b = (f / T) % B;
  const int64_t rf = b * ref_T + (ref_T == 1 ? 0 : t);
  const float* __restrict__ xf = x + f * n;
  float* __restrict__ of = out + f * n;
  const int bad = pm_load_words(xf, n, npad, s) | ref_flags[rf];
  if (bad) {
    for (int r = threadIdx.x; r < n; r += PM_THREADS) of[r] = __uint_as_float(0x7fc00000u);
    return;
  }
  pm_sort_lds<uint64_t>(s, npad);
  int dry = 0;                                          // n - n_x: the words with key <= thr_key (the same search in every thread)
  if (use_thr) {
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((uint32_t)(s[mid] >> 32) <= thr_key) lo = mid + 1;
      else hi = mid;
    }
    dry = lo;
  }
  const uint32_t* __restrict__ rk = ref_keys + rf * n;
  for (int r = threadIdx.x; r < n; r += PM_THREADS) {
    const uint32_t k = rk[r];
    const float v = (r < dry && k > thr_key) ? thr : __uint_as_float(pm_unkey(k));
    of[(uint32_t)s[r]] = v;
  }
}

// One merge pass over every group's `total` keys: runs of length L (the last one shorter) -> runs of 2 L.  A thread owns PM_VT consecutive
// outputs of one pair of runs.  grid: ceil(groups * pairs * cpp / PM_MERGE_THREADS), pairs = ceil(total / 2 L), cpp = ceil(2 L / PM_VT).
__global__ void __launch_bounds__(PM_MERGE_THREADS) pm_merge_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int64_t groups,
                                                                    int64_t total, int64_t L, int64_t pairs, int64_t cpp) {
  const int64_t id = (int64_t)blockIdx.x * PM_MERGE_THREADS + threadIdx.x;
  if (id >= groups * pairs * cpp) return;
  const int64_t g = id / (pairs * cpp), pr = (id / cpp) % pairs, d = (id % cpp) * PM_VT;
  const int64_t base = pr * 2 * L;
  const int64_t na = min(L, total - base), nb = min(L, max((int64_t)0, total - base - L));
  if (d >= na + nb) return;
  const uint32_t* __restrict__ A = src + g * total + base;
  const uint32_t* __restrict__ Bq = A + na;
  uint32_t* __restrict__ O = dst + g * total + base;
  int64_t lo = max((int64_t)0, d - nb), hi = min(d, na);
  while (lo < hi) {                                     // merge path: ai + bi = d, A first on ties
    const int64_t mid = (lo + hi) >> 1;
    if (A[mid] <= Bq[d - 1 - mid]) lo = mid + 1;
    else hi = mid;
  }
  int64_t ai = lo, bi = d - lo;
  uint32_t a = ai < na ? A[ai] : 0u, bv = bi < nb ? Bq[bi] : 0u;
  const int64_t end = min(d + PM_VT, na + nb);
  for (int64_t o = d; o < end; ++o) {
    const bool take_a = bi >= nb || (ai < na && a <= bv);
    O[o] = take_a ? a : bv;
    if (take_a) {
      ++ai;
      a = ai < na ? A[ai] : 0u;
    } else {
      ++bi;
      bv = bi < nb ? Bq[bi] : 0u;
    }
  }
}

// grid: frames (b, t).  ens (M, frames, n); P: the pooled sorted keys [frames][M n].  dynamic LDS: npad 64-bit words.
__global__ void __launch_bounds__(PM_THREADS) pm_pmm_kernel(const float* __restrict__ ens, int M, int64_t frames, const uint32_t* __restrict__ P,
                                                            int n, int npad, float* __restrict__ out) {
  extern __shared__ uint64_t pm_smem64[];
  uint64_t* s = pm_smem64;
  const int64_t f = blockIdx.x;
  const float* __restrict__ e0 = ens + f * n;
  float* __restrict__ of = out + f * n;
  int bad = 0;
  for (int i = threadIdx.x; i < npad; i += PM_THREADS) {
    uint64_t w = ~0ull;
    if (i < n) {
      double acc = 0.0;
      for (int m = 0; m < M; ++m) acc += (double)e0[(int64_t)m * frames * n + i];
      const uint32_t u = __float_as_uint((float)(acc / (double)M));
      bad |= pm_nonfinite(u);                           // any non-finite member pixel makes its fp64 sum non-finite
      w = ((uint64_t)pm_key(u) << 32) | (uint32_t)i;
    }
    s[i] = w;
  }
  if (__syncthreads_or(bad)) {
    for (int r = threadIdx.x; r < n; r += PM_THREADS) of[r] = __uint_as_float(0x7fc00000u);
    return;
  }
  pm_sort_lds<uint64_t>(s, npad);
  const uint32_t* __restrict__ Pf = P + f * (int64_t)M * n + (M >> 1);
  for (int r = threadIdx.x; r < n; r += PM_THREADS) of[(uint32_t)s[r]] = __uint_as_float(pm_unkey(Pf[(int64_t)r * M]));
}

int pm_npad(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}

int pm_check_frame(const char* who, int H, int W) {
  PD_CHECK_ARG(H >= 1 && W >= 1 && (int64_t)H * W <= PM_MAX_N,
               "%s: frames of %d x %d: 1 <= H, W and H W <= %d (the frame is sorted in LDS)", who, H, W, PM_MAX_N);
  return PD_OK;
}

bool pm_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return pa < pb + b_bytes && pb < pa + a_bytes;
}

int64_t pm_align8(int64_t v) { return (v + 7) & ~(int64_t)7; }

}  // namespace

// op 0: pd_rank_frames (no workspace: 0), op 1: pd_cdf_match with `frames` reference frames, op 2: pd_pmm with M members of `frames`
// (b, t) frames.  -1: unsupported.
extern "C" int64_t pd_pm_ws_bytes(int op, int M, int64_t frames, int H, int W) {
  if (H < 1 || W < 1 || (int64_t)H * W > PM_MAX_N || frames < 1 || op < 0 || op > 2) return -1;
  const int64_t n = (int64_t)H * W;
  if (op == 0) return frames * n > PM_MAX_TOTAL ? -1 : 0;
  if (op == 1) return frames * n > PM_MAX_TOTAL ? -1 : pm_align8(frames * n * 4) + pm_align8(frames * 4);
  if (M < 1 || M > PM_MAX_M || (double)frames * (double)M * (double)n > (double)PM_MAX_TOTAL) return -1;
  return 2 * pm_align8(frames * M * n * 4);
}

extern "C" int pd_rank_frames(const float* x, int64_t frames, int H, int W, float* sorted, int* order, pd_stream_t stream) {
  PD_CHECK_ARG(x && sorted && order, "pd_rank_frames: null pointer");
  if (int rc = pm_check_frame("pd_rank_frames", H, W)) return rc;
  PD_CHECK_ARG(pd_pm_ws_bytes(0, 1, frames, H, W) == 0, "pd_rank_frames: %lld frames (1 .. 2^31 / (H W))", (long long)frames);
  const int n = H * W, npad = pm_npad(n);
  const int64_t bytes = frames * n * 4;
  PD_CHECK_ARG(!pm_overlap(sorted, bytes, x, bytes) && !pm_overlap(order, bytes, x, bytes) && !pm_overlap(sorted, bytes, order, bytes),
               "pd_rank_frames: an output aliases an input");
  static bool lds_set[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_rank_frames", (const void*)pm_rank_kernel, PM_LDS_LIMIT, lds_set)) return rc;
  hipLaunchKernelGGL(pm_rank_kernel, dim3((unsigned)frames), dim3(PM_THREADS), (size_t)npad * 8, (hipStream_t)stream, x, n, npad, sorted,
                     order);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_cdf_match(const float* x, const float* ref, int64_t lead, int64_t B, int T, int ref_T, int H, int W, float threshold,
                            int use_threshold, float* out, void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(x && ref && out && ws, "pd_cdf_match: null pointer");
  if (int rc = pm_check_frame("pd_cdf_match", H, W)) return rc;
  PD_CHECK_ARG(lead >= 1 && B >= 1 && T >= 1 && (ref_T == T || ref_T == 1), "pd_cdf_match: x (%lld, %lld, %d) frames, ref (%lld, %d): ref holds T or 1 frames per sequence",
               (long long)lead, (long long)B, T, (long long)B, ref_T);
  PD_CHECK_ARG(!use_threshold || (threshold - threshold == 0.0f), "pd_cdf_match: the threshold must be finite");
  const int n = H * W, npad = pm_npad(n);
  const int64_t rframes = B * ref_T;
  PD_CHECK_ARG((double)lead * (double)B * (double)T * n <= (double)PM_MAX_TOTAL, "pd_cdf_match: too many frames in one call");
  const int64_t frames = lead * B * T, need = pd_pm_ws_bytes(1, 1, rframes, H, W);
  PD_CHECK_ARG(need > 0 && ws_bytes >= need && ((uintptr_t)ws & 7) == 0,
               "pd_cdf_match: the workspace holds %lld bytes (8-byte aligned), %lld are needed", (long long)ws_bytes, (long long)need);
  PD_CHECK_ARG(!pm_overlap(out, frames * n * 4, x, frames * n * 4) && !pm_overlap(out, frames * n * 4, ref, rframes * n * 4) &&
                   !pm_overlap(out, frames * n * 4, ws, need),
               "pd_cdf_match: out aliases an input");
  uint32_t* keys = (uint32_t*)ws;
  int* flags = (int*)((char*)ws + pm_align8(rframes * n * 4));
  static bool lds_set[PD_MAX_DEVICES], lds_set2[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_cdf_match", (const void*)pm_sort_keys_kernel, PM_LDS_LIMIT, lds_set)) return rc;
  if (int rc = pd_raise_lds("pd_cdf_match", (const void*)pm_match_kernel, PM_LDS_LIMIT, lds_set2)) return rc;
  hipLaunchKernelGGL(pm_sort_keys_kernel, dim3((unsigned)rframes), dim3(PM_THREADS), (size_t)npad * 4, (hipStream_t)stream, ref, (int64_t)1,
                     rframes, n, npad, keys, flags);
  PD_CHECK_LAUNCH();
  hipLaunchKernelGGL(pm_match_kernel, dim3((unsigned)frames), dim3(PM_THREADS), (size_t)npad * 8, (hipStream_t)stream, x,
                     (const uint32_t*)keys, (const int*)flags, B, T, ref_T, n, npad, pm_key_host(threshold), threshold, use_threshold ? 1 : 0,
                     out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}

extern "C" int pd_pmm(const float* ens, int M, int64_t frames, int H, int W, float* out, void* ws, int64_t ws_bytes, pd_stream_t stream) {
  PD_CHECK_ARG(ens && out && ws, "pd_pmm: null pointer");
  if (int rc = pm_check_frame("pd_pmm", H, W)) return rc;
  PD_CHECK_ARG(M >= 1 && M <= PM_MAX_M, "pd_pmm: %d members (supported: 1 .. %d)", M, PM_MAX_M);
  const int64_t need = pd_pm_ws_bytes(2, M, frames, H, W);
  PD_CHECK_ARG(need > 0, "pd_pmm: %lld frames of %d members: too many (or none) in one call", (long long)frames, M);
  PD_CHECK_ARG(ws_bytes >= need && ((uintptr_t)ws & 7) == 0, "pd_pmm: the workspace holds %lld bytes (8-byte aligned), %lld are needed",
               (long long)ws_bytes, (long long)need);
  const int n = H * W, npad = pm_npad(n);
  const int64_t total = (int64_t)M * n;
  PD_CHECK_ARG(!pm_overlap(out, frames * n * 4, ens, frames * total * 4) && !pm_overlap(out, frames * n * 4, ws, need),
               "pd_pmm: out aliases an input");
  uint32_t* buf[2] = {(uint32_t*)ws, (uint32_t*)((char*)ws + need / 2)};
  static bool lds_set[PD_MAX_DEVICES], lds_set2[PD_MAX_DEVICES];
  if (int rc = pd_raise_lds("pd_pmm", (const void*)pm_sort_keys_kernel, PM_LDS_LIMIT, lds_set)) return rc;
  if (int rc = pd_raise_lds("pd_pmm", (const void*)pm_pmm_kernel, PM_LDS_LIMIT, lds_set2)) return rc;
  hipLaunchKernelGGL(pm_sort_keys_kernel, dim3((unsigned)(frames * M)), dim3(PM_THREADS), (size_t)npad * 4, (hipStream_t)stream, ens,
                     (int64_t)M, frames, n, npad, buf[0], (int*)nullptr);
  PD_CHECK_LAUNCH();
  int cur = 0;
  for (int64_t L = n; L < total; L *= 2) {
    const int64_t pairs = (total + 2 * L - 1) / (2 * L), cpp = (2 * L + PM_VT - 1) / PM_VT;
    const int64_t threads = frames * pairs * cpp;
    hipLaunchKernelGGL(pm_merge_kernel, dim3((unsigned)((threads + PM_MERGE_THREADS - 1) / PM_MERGE_THREADS)), dim3(PM_MERGE_THREADS), 0,
                       (hipStream_t)stream, (const uint32_t*)buf[cur], buf[cur ^ 1], frames, total, L, pairs, cpp);
    PD_CHECK_LAUNCH();
    cur ^= 1;
  }
  hipLaunchKernelGGL(pm_pmm_kernel, dim3((unsigned)frames), dim3(PM_THREADS), (size_t)npad * 8, (hipStream_t)stream, ens, M, frames,
                     (const uint32_t*)buf[cur], n, npad, out);
  PD_CHECK_LAUNCH();
  return PD_OK;
}
